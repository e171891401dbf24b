"""lapwarm_seeded_ragged on the MI355X: the seeded solve of a ragged batch, one solver launch per kernel
configuration (WarmStartPipeline.seeded_ragged, and solve_many on top of it).

The yardstick is seeded_batch of every instance alone (batch 1): x, y and ret must be identical, stats identical
in every slot but the time and stamp slots (13, 14, 16 ..), without any tolerance -- an instance runs under the
instantiation it would get alone.  Where tests/golden/seeded_cases.npz holds cases of several sizes, the
reference's recorded assignments are a second yardstick.  Padding cells of C and of the seeds hold NaN and
padding entries of x, y must come back -1."""
import ctypes as ct
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAT_SLOTS = list(range(13)) + [15]  # everything but kernel / serial ticks and the stamp block
LADDER = [1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 128, 129, 255, 256, 257]


@functools.lru_cache(maxsize=None)
def pipe():
    import torch

    from gnn import OneGNN, WarmStartPipeline
    torch.manual_seed(0)
    return WarmStartPipeline(OneGNN(21, 64, 2).cuda().eval())


def reduction_seeds(C):
    """Row minima, then the column minima of what is left: feasible, with a tight edge in every row."""
    u = C.min(axis=1)
    return u, (C - u[:, None]).min(axis=0)


def make_pack(mats, ld=0, N=None, descending=False):
    """A RaggedPack laid out here, NaN in every cell that belongs to no instance: packed (ld = 0) or with a common
    row stride; `descending` puts instance 0 at the highest address."""
    import torch

    from gnn.features import RaggedPack
    sizes = [m.shape[0] for m in mats]
    N = N or max(sizes)
    spans = [(n - 1) * (ld or n) + n for n in sizes]
    order = range(len(mats))[::-1] if descending else range(len(mats))
    offsets, total = [0] * len(mats), 1  # one leading NaN: odd element offsets, 8-byte alignment only
    for b in order:
        offsets[b] = total
        total += spans[b] + 1
    buf = np.full(total, np.nan)
    for m, o, n in zip(mats, offsets, sizes):
        stride = ld or n
        for i in range(n):
            buf[o + i * stride:o + i * stride + n] = m[i]
    C = torch.from_numpy(buf).cuda()
    return RaggedPack(C, torch.tensor(offsets, dtype=torch.int64).cuda(), torch.tensor(sizes, dtype=torch.int32).cuda(),
                      None, None, ld, N, sizes)


def padded_seeds(seeds, N):
    import torch
    out = np.full((2, len(seeds), N), np.nan)
    for b, (u, v) in enumerate(seeds):
        out[0, b, :len(u)], out[1, b, :len(v)] = u, v
    t = torch.from_numpy(out).cuda()
    return t[0].contiguous(), t[1].contiguous()


def solve_alone(C, u, v, eps=1e-12):
    import torch
    x, y, ret, stats = pipe().seeded_batch(torch.from_numpy(C).cuda()[None], torch.from_numpy(u).cuda()[None],
                                           torch.from_numpy(v).cuda()[None], eps)
    return x[0].cpu().numpy(), y[0].cpu().numpy(), int(ret[0]), stats[0].cpu().numpy()


def solve_ragged(mats, seeds, eps=1e-12, **layout):
    p = make_pack(mats, **layout)
    u, v = padded_seeds(seeds, p.N)
    x, y, ret, stats = pipe().seeded_ragged(p, u, v, eps)
    return x.cpu().numpy(), y.cpu().numpy(), ret.cpu().numpy(), stats.cpu().numpy()


def check_against_alone(mats, seeds, got, eps=1e-12):
    x, y, ret, stats = got
    assert x.dtype == np.int64 and y.dtype == np.int64 and ret.dtype == np.int32 and stats.dtype == np.int64
    for b, (C, (u, v)) in enumerate(zip(mats, seeds)):
        n = C.shape[0]
        xa, ya, ra, sa = solve_alone(C, u, v, eps)
        assert ret[b] == ra, (b, n, ret[b], ra)
        assert np.array_equal(x[b, :n], xa) and np.array_equal(y[b, :n], ya), (b, n)
        assert (x[b, n:] == -1).all() and (y[b, n:] == -1).all(), (b, n)
        assert np.array_equal(stats[b, STAT_SLOTS], sa[STAT_SLOTS]), (b, n, stats[b, :16], sa[:16])
        if ra == 0:
            assert sorted(xa.tolist()) == list(range(n))
    return stats[:, 0]


def uniform_mats(sizes, seed):
    rs = np.random.RandomState(seed)
    return [rs.uniform(0.0, 1.0, (n, n)) for n in sizes]


# ----------------------------------------------------------------------------------------- the size ladder
@pytest.mark.parametrize("layout", ("packed", "padded"))
def test_size_ladder_in_one_call(layout):
    sizes = list(np.random.RandomState(3).permutation(LADDER))
    mats = uniform_mats(sizes, 31)
    seeds = [reduction_seeds(C) for C in mats]
    N = max(sizes)
    kw = dict(ld=N + 3) if layout == "padded" else {}
    check_against_alone(mats, seeds, solve_ragged(mats, seeds, **kw))


# ------------------------------------------------------------------------ every solver instantiation
# One size or two per kernel configuration of the larger sizes, the last eligible size among them: 512 and 1024
# threads at one position per lane, then two and four positions per lane (the odd sizes above 1024 and 2048).
CONFIG_SIZES = [511, 513, 1023, 1025, 2047, 2049, 3631]


@functools.lru_cache(maxsize=None)
def config_cases():
    """The matrices, their seeds and seeded_batch of each alone: computed once, shared by the two layouts."""
    mats = uniform_mats(CONFIG_SIZES, 33)
    seeds = [reduction_seeds(C) for C in mats]
    return mats, seeds, [solve_alone(C, u, v) for C, (u, v) in zip(mats, seeds)]


@pytest.mark.parametrize("layout", ("packed", "padded"))
def test_one_size_per_larger_configuration_in_one_call(layout):
    p = pipe()
    assert all(p.ragged_solve_eligible(n) for n in CONFIG_SIZES) and not p.ragged_solve_eligible(3633)
    group_of = (ct.c_int * len(CONFIG_SIZES))()
    assert p.lib.lapwarm_seeded_ragged_groups((ct.c_int * len(CONFIG_SIZES))(*CONFIG_SIZES), len(CONFIG_SIZES),
                                              group_of) == 4
    assert list(group_of) == [0, 1, 1, 2, 2, 3, 3]
    mats, seeds, alone = config_cases()
    kw = dict(ld=max(CONFIG_SIZES) + 3) if layout == "padded" else {}
    x, y, ret, stats = solve_ragged(mats, seeds, **kw)
    for b, (n, (xa, ya, ra, sa)) in enumerate(zip(CONFIG_SIZES, alone)):
        assert ra == 0 and ret[b] == 0, (n, ra, ret[b])
        assert np.array_equal(x[b, :n], xa) and np.array_equal(y[b, :n], ya), n
        assert (x[b, n:] == -1).all() and (y[b, n:] == -1).all(), n
        assert np.array_equal(stats[b, STAT_SLOTS], sa[STAT_SLOTS]), (n, stats[b, :16], sa[:16])


# ----------------------------------------------------------------------------- configuration boundaries
def configuration_boundaries():
    """Neighbouring eligible sizes that lapwarm_seeded_ragged_groups puts into different groups, over every size the
    entry takes: (n, n + 1) below the first size it refuses, (n, n + 2) among the odd sizes above it."""
    lib = pipe().lib
    sizes = [n for n in range(1, 4429) if pipe().ragged_solve_eligible(n)]
    group_of = (ct.c_int * len(sizes))()
    count = lib.lapwarm_seeded_ragged_groups((ct.c_int * len(sizes))(*sizes), len(sizes), group_of)
    assert count >= 2
    return [(n, m) for n, m, a, b in zip(sizes, sizes[1:], group_of, group_of[1:]) if a != b]


def test_either_side_of_every_configuration_boundary_in_one_call():
    pairs = configuration_boundaries()
    assert len(pairs) >= 4 and (64, 65) in pairs and (256, 257) in pairs, pairs
    assert (1023, 1025) in pairs and (2047, 2049) in pairs, pairs
    lib = pipe().lib
    for k, pair in enumerate(pairs):
        assert lib.lapwarm_seeded_ragged_groups((ct.c_int * 2)(*pair), 2, (ct.c_int * 2)()) == 2  # two launches
        mats = uniform_mats(pair, 40 + k)
        seeds = [reduction_seeds(C) for C in mats]
        check_against_alone(mats, seeds, solve_ragged(mats, seeds))


# -------------------------------------------------------------------------------------- seeds per branch
def test_seeds_that_take_each_branch_mixed_in_one_call():
    import torch
    sizes = [40, 96, 130]
    base = uniform_mats(sizes, 50)
    mats, seeds = [], []
    model = pipe().predict_ragged(base)
    for C, (um, vm) in zip(base, model):
        n = C.shape[0]
        _, uo, vo, ro = pipe().optimal_duals_batch(torch.from_numpy(C).cuda()[None])
        assert int(ro[0]) == 0
        for u, v in ((np.zeros(n), np.zeros(n)),                    # no tight edge: the quality-gate fallback
                     reduction_seeds(C),                            # greedy, then shortest paths
                     (uo[0].cpu().numpy(), vo[0].cpu().numpy()),    # optimal duals: all matched, no path
                     (um.cpu().numpy(), vm.cpu().numpy())):         # the model's own prediction
            mats.append(C)
            seeds.append((u, v))
    order = np.random.RandomState(5).permutation(len(mats))
    mats, seeds = [mats[k] for k in order], [seeds[k] for k in order]
    branch = check_against_alone(mats, seeds, solve_ragged(mats, seeds))
    print("branches:", branch.tolist())
    assert len(set(branch.tolist())) >= 2


# ------------------------------------------------------------------------------------------------- ties
def test_integer_costs_keep_the_lowest_index_tie_breaking():
    rs = np.random.RandomState(61)
    mats, seeds = [], []
    for n in (17, 64, 130):
        C = rs.randint(0, 10, (n, n)).astype(np.float64)
        for s in ((np.zeros(n), np.zeros(n)), reduction_seeds(C)):
            mats.append(C)
            seeds.append(s)
    check_against_alone(mats, seeds, solve_ragged(mats, seeds))


# ------------------------------------------------------------------------------------- degenerate batches
def test_batch_of_one():
    mats = uniform_mats([33], 70)
    seeds = [reduction_seeds(mats[0])]
    check_against_alone(mats, seeds, solve_ragged(mats, seeds))


def test_all_sizes_equal_is_seeded_batch_of_the_stacked_batch():
    import torch
    mats = uniform_mats([48] * 4, 71)
    seeds = [reduction_seeds(C) for C in mats]
    x, y, ret, stats = solve_ragged(mats, seeds)
    u = torch.from_numpy(np.stack([s[0] for s in seeds])).cuda()
    v = torch.from_numpy(np.stack([s[1] for s in seeds])).cuda()
    xs, ys, rs_, ss = pipe().seeded_batch(torch.from_numpy(np.stack(mats)).cuda(), u, v)
    assert np.array_equal(x, xs.cpu().numpy()) and np.array_equal(y, ys.cpu().numpy())
    assert np.array_equal(ret, rs_.cpu().numpy())
    assert np.array_equal(stats[:, STAT_SLOTS], ss.cpu().numpy()[:, STAT_SLOTS])


def test_offsets_in_descending_order_of_address():
    sizes = [65, 5, 130, 32]
    mats = uniform_mats(sizes, 72)
    seeds = [reduction_seeds(C) for C in mats]
    p = make_pack(mats, descending=True)
    off = p.offsets.tolist()
    assert off == sorted(off, reverse=True)
    check_against_alone(mats, seeds, solve_ragged(mats, seeds, descending=True))


# ------------------------------------------------------------------------------- the reference's records
def test_golden_seeded_cases_as_ragged_calls(seeded_cases):
    """The recorded cases, all sizes of one eps in one call: ret, and x, y where the reference solved."""
    by_eps = {}
    for k in range(len(seeded_cases)):
        c = seeded_cases.case(k)
        by_eps.setdefault(c["eps"], []).append(c)
    # (one call per eps, which is an argument of the call; at least one of them mixes sizes)
    assert len(by_eps) >= 2 and max(len({c["n"] for c in cases}) for cases in by_eps.values()) >= 2
    n_ok = n_bad = 0
    for eps, cases in by_eps.items():
        x, y, ret, _ = solve_ragged([c["C"] for c in cases], [(c["u"], c["v"]) for c in cases], eps)
        for b, c in enumerate(cases):
            n = c["n"]
            assert ret[b] == c["ret"], c["label"]
            assert (x[b, n:] == -1).all() and (y[b, n:] == -1).all(), c["label"]
            if c["ret"] == 0:
                assert np.array_equal(x[b, :n], c["x"]) and np.array_equal(y[b, :n], c["y"]), c["label"]
                n_ok += 1
            else:
                n_bad += 1
    assert n_ok > 200 and n_bad >= 5


# ------------------------------------------------------------------------------------------ launch count
def test_solve_many_makes_one_ragged_call_and_keeps_the_old_path_for_helper_sizes(monkeypatch):
    import torch
    p = pipe()
    sizes = [300, 5, 64, 600, 33, 129, 65, 513, 200, 257, 100, 400]
    assert len(set(sizes)) == 12 and all(p.ragged_solve_eligible(n) for n in sizes)
    assert not p.ragged_solve_eligible(1024)
    costs = uniform_mats(sizes + [1024], 80)
    calls = {"ragged": 0, "batched": 0}
    ragged, batched = p.lib.lapwarm_seeded_ragged, p.lib.lapwarm_seeded_batched

    def count(name, fn):
        def wrapped(*args):
            calls[name] += 1
            return fn(*args)
        return wrapped
    monkeypatch.setattr(p.lib, "lapwarm_seeded_ragged", count("ragged", ragged))
    monkeypatch.setattr(p.lib, "lapwarm_seeded_batched", count("batched", batched))

    got = p.solve_many(costs[:12])
    assert calls == {"ragged": 1, "batched": 0}
    got_13 = p.solve_many(costs)
    assert calls == {"ragged": 2, "batched": 1}
    monkeypatch.undo()
    # a threads_hint does not reach the ragged launches: such a pipeline keeps the per-size path
    from gnn import WarmStartPipeline
    hinted = WarmStartPipeline(p.model, threads_hint=256)
    monkeypatch.setattr(p.lib, "lapwarm_seeded_ragged", count("ragged", ragged))
    monkeypatch.setattr(p.lib, "lapwarm_seeded_batched", count("batched", batched))
    assert len(hinted.solve_many(costs[1:3])) == 2
    assert calls == {"ragged": 2, "batched": 3}
    monkeypatch.undo()

    # what solve_many returned before: the model's seeds, then seeded_batch of every size on its own
    for out, n_inst in ((got, 12), (got_13, 13)):
        assert len(out) == n_inst
        _, u, v = p._predict_ragged(costs[:n_inst])
        for b in range(n_inst):
            n = costs[b].shape[0]
            g = out[b]
            # (the seeds it returns are the seeds it solved with; a second forward is held to the project's 1e-5)
            assert g["u"].shape == (n,) and (g["u"] - u[b, :n]).abs().max().item() <= 1e-5, (b, n)
            assert g["v"].shape == (n,) and (g["v"] - v[b, :n]).abs().max().item() <= 1e-5, (b, n)
            x, y, ret, stats = p.seeded_batch(torch.from_numpy(costs[b]).cuda()[None], g["u"][None], g["v"][None])
            assert g["x"].shape == (n,) and g["x"].dtype == torch.int64 and g["y"].dtype == torch.int64
            assert g["ret"].dtype == torch.int32 and g["stats"].dtype == torch.int64 and g["stats"].shape == (32,)
            assert g["u"].dtype == torch.float64 and g["v"].dtype == torch.float64
            assert torch.equal(g["x"], x[0]) and torch.equal(g["y"], y[0]) and torch.equal(g["ret"], ret[0]), (b, n)
            assert torch.equal(g["stats"][STAT_SLOTS], stats[0][STAT_SLOTS]), (b, n)
