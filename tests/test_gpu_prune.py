"""The pruned exact solve on the device (csrc/prune_price.hip, WarmStartPipeline.lapjv_pruned_ragged): one grow
step against the NumPy restatement bit for bit, the whole solve against tests/golden/prune_cases.npz, the
certificate recomputed in NumPy, the return codes and run-to-run equality."""
import numpy as np
import pytest

from host_common import bits_equal, padded, shared_pipe as pipe, torch_cuda  # noqa: F401
from prune_common import CASES, case_matrix, family_matrix, grow, load_fixture, solve_pruned, to_csr

pytestmark = pytest.mark.gpu


def make_pack(pipe, mats, layout):
    from gnn.features import ragged_pack
    if layout == "packed":
        return ragged_pack(mats, pipe.device)
    width = max(m.shape[0] for m in mats) + 3
    return ragged_pack(padded(mats, width), pipe.device, sizes=[m.shape[0] for m in mats])


def device_grow(pipe, mats, m, layout, keys=None, xs=None, rows=None):
    """One grow step of a batch; per instance (ii, kk, cc), then added, viol and ret."""
    import torch
    from gnn.pipeline import sparse_pack
    pack = make_pack(pipe, mats, layout)
    B, N = len(mats), pack.N

    def wide(vectors, dtype):
        if vectors is None:
            return None
        host = np.zeros((B, N), dtype=dtype)
        for b, vec in enumerate(vectors):
            host[b, :len(vec)] = vec
        return torch.from_numpy(host).to(pipe.device)

    csr = None
    if rows is not None:
        csr = sparse_pack([(c.shape[0],) + to_csr(c, r) for c, r in zip(mats, rows)], pipe.device)
    nxt, counts = pipe.prune_grow(pack, m, key=wide(keys, np.float64), x=wide(xs, np.int32), csr=csr)
    added, viol, ret = pipe.prune_counts(counts, B)
    cc, kk, ii = nxt.cc.cpu().numpy(), nxt.kk.cpu().numpy(), nxt.ii.cpu().numpy()
    noff, roff = nxt.nnz_offsets.tolist(), nxt.row_offsets.tolist()
    out = []
    for b, c in enumerate(mats):
        n = c.shape[0]
        row_starts = ii[roff[b]:roff[b] + n + 1]
        out.append((row_starts, kk[noff[b]:noff[b] + row_starts[-1]], cc[noff[b]:noff[b] + row_starts[-1]]))
    return out, added, viol, ret


def check_step(got, mats, m, keys, bounds, rows):
    out, added, viol, ret = got
    for b, C in enumerate(mats):
        n = C.shape[0]
        cur = rows[b] if rows is not None else [np.array([i]) for i in range(n)]
        want_rows, want_viol = grow(C, cur, None if keys is None else keys[b], None if bounds is None else bounds[b], m)
        cc, ii, kk = to_csr(C, want_rows)
        tag = (b, n, m)
        assert ret[b] == 0 and viol[b] == want_viol, tag
        assert added[b] == int(ii[-1]) - (sum(len(r) for r in rows[b]) if rows is not None else 0), tag
        assert np.array_equal(out[b][0], ii), tag
        assert np.array_equal(out[b][1], kk), tag
        assert bits_equal(out[b][2], cc), tag


ROUND0_SIZES = (1, 2, 5, 17, 63, 64, 65, 257)  # the second instance of the packed batch lies at an odd 8-byte offset


@pytest.mark.parametrize("layout", ["packed", "padded"])
@pytest.mark.parametrize("k", [1, 16, 64, 256])
def test_round0_step_matches_the_restatement(pipe, k, layout):
    fams = ("uniform", "integer", "metric", "lowrank", "constant", "uniform", "integer", "metric")
    mats = [family_matrix(f, n, 31 + n) for f, n in zip(fams, ROUND0_SIZES)]
    mats.append(family_matrix("constant", 70, 0))  # all ties: the lower columns win
    if k == 256:
        mats.append(family_matrix("uniform", 300, 5))  # 256 of 299
    check_step(device_grow(pipe, mats, k, layout), mats, k, None, None, None)
    rng = np.random.default_rng(k)
    seeds = [rng.random(c.shape[0]) * c.mean() for c in mats]
    check_step(device_grow(pipe, mats, k, layout, keys=seeds), mats, k, seeds, None, None)


def test_round0_step_where_the_row_loop_repeats(pipe):
    C = family_matrix("integer", 2049, 3)  # many ties, 2049 columns over 320 threads
    check_step(device_grow(pipe, [C], 16, "packed"), [C], 16, None, None, None)


def pricing_instances(m):
    """(C, rows, v, x) per instance: rows from a round 0, then rows of more than 64 entries, a full row, a row with
    exactly m eligible entries and one with m + 1."""
    rng = np.random.default_rng(100 + m)
    out = []
    for family, n in (("uniform", 65), ("metric", 130), ("constant", 64), ("integer", 257), ("lowrank", 2)):
        C = family_matrix(family, n, 77)
        rows, _ = grow(C, [np.array([i]) for i in range(n)], None, None, min(m, 8))
        x = rng.permutation(n)
        v = rng.random(n) * 0.2 * C.mean()
        if family == "constant":  # row 0 is bounded by 8 and every absent key is 7: all tie, the lowest m win
            x, v = np.arange(n), np.zeros(n)
            v[0] = -1.0
        out.append((C, rows, v, x))
    n = 130
    C = 50.0 + family_matrix("uniform", n, 78)
    x, v = np.arange(n), np.zeros(n)
    rows = [np.array([i]) for i in range(n)]
    rows[0] = np.arange(n)                          # full already
    rows[1] = np.union1d([1], np.arange(20, 95))    # more than 64 entries
    for i, count in ((2, m), (3, m + 1), (4, 0)):   # bound 10: exactly m, m + 1 and no absent entries below it
        C[i, i] = 10.0
        cols = rng.choice(np.setdiff1d(np.arange(n), [i]), size=min(count, n - 1), replace=False)
        C[i, cols] = rng.integers(1, 4, size=cols.size).astype(np.float64)
    C[1, 1] = 60.0  # row 1 is bounded above every cost: all its 54 absent entries are eligible
    out.append((C, rows, v, x))
    return out


@pytest.mark.parametrize("layout", ["packed", "padded"])
@pytest.mark.parametrize("m", [1, 16, 64])
def test_pricing_step_matches_the_restatement(pipe, m, layout):
    inst = pricing_instances(m)
    mats, rows = [t[0] for t in inst], [t[1] for t in inst]
    vs, xs = [t[2] for t in inst], [t[3] for t in inst]
    bounds = [C[np.arange(C.shape[0]), x] - v[x] for C, _, v, x in inst]
    got = device_grow(pipe, mats, m, layout, keys=vs, xs=xs, rows=rows)
    check_step(got, mats, m, vs, bounds, rows)
    C, r, v, x = inst[-1]
    lens = np.diff(got[0][-1][0])
    assert lens[0] == 130 and lens[1] == 76 + min(m, 54) and lens[2] == 1 + min(m, 129) and lens[4] == 1
    assert lens[3] == 1 + min(m, 129)  # m of the m + 1


def solve(pipe, mats, k, layout="packed", **kw):
    out = pipe.lapjv_pruned_ragged(make_pack(pipe, mats, layout), k, **kw)
    return {key: t.cpu().numpy() for key, t in out.items()}


def check_against_fixture(out, b, label):
    f = load_fixture()[label]
    n = f["n"]
    assert out["ret"][b] == 0 and out["viol_last"][b] == 0, label
    assert out["rounds"][b] == len(f["trace"]) and out["nnz"][b] == f["trace"][-1][0], (label, out["rounds"][b])
    assert np.array_equal(out["x"][b, :n], f["x"]) and np.all(out["x"][b, n:] == -1), label
    assert np.array_equal(out["y"][b, :n], np.argsort(f["x"])) and np.all(out["y"][b, n:] == -1), label
    assert bits_equal(out["v"][b, :n], f["v"]) and np.all(out["v"][b, n:] == 0.0), label
    C = case_matrix(label)
    assert bits_equal(out["u"][b, :n], C[np.arange(n), f["x"]] - f["v"][f["x"]]) and np.all(out["u"][b, n:] == 0.0)
    assert bits_equal(out["cost"][b:b + 1], [f["cost"]]), label


@pytest.mark.parametrize("label", [c[0] for c in CASES])
def test_whole_solve_alone_matches_the_fixture(pipe, label):
    check_against_fixture(solve(pipe, [case_matrix(label)], load_fixture()[label]["k"]), 0, label)


@pytest.mark.parametrize("layout", ["packed", "padded"])
def test_whole_solve_of_a_mixed_batch_matches_the_fixture(pipe, layout):
    labels = [c[0] for c in CASES if c[3] == 16]
    assert len({load_fixture()[s]["n"] for s in labels}) >= 8
    mats = [case_matrix(s) for s in labels]
    out = solve(pipe, mats, 16, layout)
    for b, label in enumerate(labels):
        check_against_fixture(out, b, label)  # which is what the instance gives alone (the test above)
    again = solve(pipe, mats, 16, layout)
    for key in out:
        assert out[key].tobytes() == again[key].tobytes(), key


def device_lapmod(pipe):
    from gnn.pipeline import sparse_pack

    def lapmod(n, cc, ii, kk):
        out = pipe.lapmod_ragged(sparse_pack([(n, cc, ii, kk)], pipe.device), 3, want_stats=False)
        assert int(out["ret"][0]) == 0
        return out["x"][0, :n].cpu().numpy(), out["v"][0, :n].cpu().numpy()
    return lapmod


@pytest.mark.parametrize("family,n,k", [("integer", 150, 4), ("uniform", 131, 2), ("lowrank", 97, 8)])
def test_certificate_recomputed_in_numpy(pipe, torch_cuda, family, n, k):
    C = family_matrix(family, n, 1234)
    out = solve(pipe, [C], k)
    want = solve_pruned(C, k, device_lapmod(pipe))
    assert out["ret"][0] == 0 and want["ret"] == 0 and out["rounds"][0] == want["rounds"] > 1
    x, u, v = out["x"][0], out["u"][0], out["v"][0]
    assert np.array_equal(x, want["x"]) and bits_equal(v, want["v"]) and bits_equal(u, C[np.arange(n), x] - v[x])
    assert np.array_equal(np.sort(x), np.arange(n))
    absent = np.ones((n, n), dtype=bool)
    for i, r in enumerate(want["rows"]):
        absent[i, r] = False
    assert int(out["nnz"][0]) == n * n - absent.sum()
    assert np.all((C - v[None, :] >= u[:, None])[absent])  # no absent entry prices in
    # ... and the entries that are present are dual feasible up to rounding, so the duals bound the optimum
    assert np.all(C - v[None, :] - u[:, None] >= -1e-9 * max(1.0, C.max()))
    assert abs(out["cost"][0] - (u.sum() + v.sum())) <= 1e-9 * max(1.0, abs(out["cost"][0]))
    if family == "integer":
        xd, _, ret, _ = pipe.lapjv_batch(torch_cuda.from_numpy(C[None]).to(pipe.device), want_stats=False)
        assert int(ret[0]) == 0 and out["cost"][0] == C[np.arange(n), xd[0].cpu().numpy()].sum()


def test_uncertified_and_inadmissible_instances(pipe):
    hard = case_matrix("lowrank_n200_k16")  # seven rounds in the fixture
    good = [case_matrix("metric_n257_k16"), case_matrix("integer_n64_k16")]
    bad = []
    for value in (1e6, -1.0, np.inf, np.nan):
        C = family_matrix("uniform", 40, 9)
        C[17, 23] = value
        bad.append(C)
    mats = [good[0]] + bad + [good[1], hard]
    out = solve(pipe, mats, 16, max_rounds=1)
    assert out["ret"].tolist() == [2, 3, 3, 3, 3, 0, 2]
    for b in (1, 2, 3, 4):
        assert np.all(out["x"][b] == -1) and np.all(out["y"][b] == -1) and out["cost"][b] == np.inf
        assert out["rounds"][b] == 0 and np.all(out["u"][b] == 0.0) and np.all(out["v"][b] == 0.0)
    for b in (0, 6):  # a valid permutation that is not proven optimal
        n = mats[b].shape[0]
        x = out["x"][b, :n]
        assert np.array_equal(np.sort(x), np.arange(n)) and np.array_equal(out["y"][b, :n], np.argsort(x))
        assert out["rounds"][b] == 1 and out["viol_last"][b] > 0
        assert out["cost"][b] >= load_fixture()["metric_n257_k16" if b == 0 else "lowrank_n200_k16"]["cost"]
    check_against_fixture(out, 5, "integer_n64_k16")  # untouched by its neighbours
    full = solve(pipe, mats, 16)
    assert full["ret"].tolist() == [0, 3, 3, 3, 3, 0, 0]
    check_against_fixture(full, 0, "metric_n257_k16")
    check_against_fixture(full, 6, "lowrank_n200_k16")
    # the caller of solve_pruned_many always gets the optimum
    res = pipe.solve_pruned_many([hard, good[1]], k=16, use_model=False, max_rounds=1)
    f = load_fixture()["lowrank_n200_k16"]
    assert res[0]["ret"] == 2 and res[0]["fallback"] and not res[1]["fallback"]
    assert np.array_equal(res[0]["x"].cpu().numpy(), f["x"])  # the optimum is unique
    assert abs(float(res[0]["cost"]) - f["cost"]) <= 1e-12 * f["cost"] * 200
    assert float(res[1]["cost"]) == load_fixture()["integer_n64_k16"]["cost"]


@pytest.mark.parametrize("label", ["metric_n257_k16", "integer_n64_k16", "lowrank_n90_k16"])
def test_column_minima_as_seed_give_the_same_certified_cost(pipe, torch_cuda, label):
    C = case_matrix(label)
    n = C.shape[0]
    pack = make_pack(pipe, [C], "packed")
    seed = torch_cuda.from_numpy(C.min(axis=0)[None]).to(pipe.device)
    out = {key: t.cpu().numpy() for key, t in pipe.lapjv_pruned_ragged(pack, 16, seed=seed).items()}
    f = load_fixture()[label]
    assert out["ret"][0] == 0 and out["viol_last"][0] == 0
    assert bits_equal(out["cost"], [f["cost"]])
    if label != "integer_n64_k16":
        assert np.array_equal(out["x"][0, :n], f["x"])
    rows, _ = grow(C, [np.array([i]) for i in range(n)], C.min(axis=0), None, 16)
    if out["rounds"][0] == 1:
        assert out["nnz"][0] == sum(len(r) for r in rows)


def test_lap_front_end(pipe):
    import lap
    C = case_matrix("metric_n63_k4")
    f = load_fixture()["metric_n63_k4"]
    opt, x, y = lap.lapjv_pruned(C, k=4)
    assert opt == f["cost"] and np.array_equal(x, f["x"]) and np.array_equal(y, np.argsort(f["x"]))
    assert x.dtype == np.int32 and y.dtype == np.int32
    big = C.copy()
    big[3, 4] = 2e6  # LAPMOD refuses it: the dense route answers
    res = lap.lapjv_pruned_many([C, big], k=4, v=[C.min(axis=0), None])
    assert res[0][0] == f["cost"] and np.array_equal(np.sort(res[1][1]), np.arange(63))
    assert lap.lapjv_pruned(C, k=4, return_cost=False)[0].tolist() == f["x"].tolist()


@pytest.mark.parametrize("m", [16, 256])
def test_pricing_step_where_the_row_loop_repeats(pipe, m):
    """n = 2049: 320 threads hold 7 columns each, the bitmap spans 65 words, and with m = 256 most rows have more
    than 256 eligible entries, so the radix select runs in a pricing step too."""
    n = 2049
    C = family_matrix("integer", n, 4)
    rng = np.random.default_rng(m)
    rows, _ = grow(C, [np.array([i]) for i in range(n)], None, None, 4)
    rows[7] = np.arange(n)                           # full already
    rows[8] = np.union1d([8], np.arange(100, 1500))  # spans several chunks of columns
    x, v = rng.permutation(n), rng.random(n) * 5.0
    bound = C[np.arange(n), x] - v[x]
    got = device_grow(pipe, [C], m, "packed", keys=[v], xs=[x], rows=[rows])
    check_step(got, [C], m, [v], [bound], [rows])
    gained = np.diff(got[0][0][0]) - np.array([len(r) for r in rows])
    assert gained[7] == 0 and gained.max() == m
    if m == 256:
        eligible = ((C - v[None, :]) < bound[:, None]).sum(axis=1)
        assert np.sum(eligible > 256 + 5) > n // 2  # (at most 5 of them are present already)


def test_grow_steps_with_sixteen_columns_per_thread(pipe, torch_cuda):
    """n = 8200 (above 8192: 1024 threads, up to 9 of the 16 column slots of a thread in use).  All row starts, viol
    and added are checked; kk and cc on a sample of rows, against the restatement applied to those rows."""
    from gnn.features import ragged_pack
    from gnn.pipeline import sparse_pack
    n, k = 8200, 16
    rng = np.random.default_rng(8200)
    C = rng.integers(1, 101, size=(n, n)).astype(np.float64)
    sample = np.unique(np.r_[0, 1, 8191, n - 1, rng.integers(0, n, size=40)])
    pack = ragged_pack([C], pipe.device)

    def step(**kw):
        nxt, counts = pipe.prune_grow(pack, k, **kw)
        added, viol, ret = pipe.prune_counts(counts, 1)
        assert ret == [0]
        return nxt.ii.cpu().numpy(), nxt.kk.cpu().numpy(), nxt.cc.cpu().numpy(), added[0], viol[0]

    def check_rows(ii, kk, cc, want_rows):
        for i, want in zip(sample, want_rows):
            assert np.array_equal(kk[ii[i]:ii[i + 1]], want), i
            assert bits_equal(cc[ii[i]:ii[i + 1]], C[i, want]), i

    ii, kk, cc, added, viol = step()
    assert np.array_equal(ii, np.arange(n + 1) * (k + 1)) and added == n * (k + 1) and viol == n * (n - 1)
    diag = [np.array([i]) for i in sample]
    want0, _ = grow(C[sample], diag, None, None, k)
    check_rows(ii, kk[:ii[n]], cc[:ii[n]], want0)

    x, v = rng.permutation(n), rng.random(n) * 3.0
    bound = C[np.arange(n), x] - v[x]
    csr = sparse_pack([(n, cc[:ii[n]], ii, kk[:ii[n]])], pipe.device)
    to_dev = lambda a: torch_cuda.from_numpy(np.ascontiguousarray(a)[None]).to(pipe.device)  # noqa: E731
    ii2, kk2, cc2, added2, viol2 = step(key=to_dev(v), x=to_dev(x.astype(np.int32)), csr=csr)
    below = (C - v[None, :]) < bound[:, None]
    count = below.sum(axis=1) - below[np.repeat(np.arange(n), k + 1), kk[:ii[n]]].reshape(n, k + 1).sum(axis=1)
    assert viol2 == count.sum() and np.array_equal(np.diff(ii2), (k + 1) + np.minimum(k, count))
    assert added2 == np.minimum(k, count).sum() and count.max() > k
    want1, _ = grow(C[sample], [kk[ii[i]:ii[i + 1]].astype(np.int64) for i in sample], v, bound[sample], k)
    check_rows(ii2, kk2[:ii2[n]], cc2[:ii2[n]], want1)


def test_solve_pruned_many_with_the_model_seed(pipe):
    """The default route: round 0 seeded with predict_ragged's v_hat (the shared pipeline's model).  Whatever the
    seed keeps, the caller gets the optimum."""
    labels = [c[0] for c in CASES if c[3] == 16]
    res = pipe.solve_pruned_many([case_matrix(s) for s in labels], k=16)
    for r, label in zip(res, labels):
        f = load_fixture()[label]
        x = r["x"].cpu().numpy()
        assert np.array_equal(np.sort(x), np.arange(f["n"])) and np.array_equal(r["y"].cpu().numpy(), np.argsort(x))
        assert r["ret"] in (0, 2) and r["fallback"] == (r["ret"] == 2) and r["rounds"] >= 1, label
        if f["family"] in ("integer", "constant"):
            assert float(r["cost"]) == f["cost"], label  # integer sums are exact in any order
        else:
            assert np.array_equal(x, f["x"]), label      # the optimum is unique
            if not r["fallback"]:
                assert float(r["cost"]) == f["cost"], label  # the same serial sum
    assert sum(r["ret"] == 0 for r in res) >= len(res) // 2  # the seeded round 0 is not useless
