"""The ragged dual utilities without a GPU: the ABI surface of the four new entries and their argument errors, the
fixture tests/golden/dual_seeds_cases.npz against plain NumPy statements of its formulas (which pins the fixture
and the two-read form of gmin the device round uses), the stop cases the multi-round tests rest on, and the
argument errors of every new Python entry, raised before any device work."""
import ctypes as ct
import inspect

import numpy as np
import pytest

from dual_seeds_common import (case_key, case_names, cases, combos, matrix, np_project, np_reduce,
                               np_seed_row_col_minima, quiet_warnings, same)
from host_common import lib  # noqa: F401


def test_workspace_query(lib):
    q = lib.lapwarm_ragged_duals_workspace_bytes
    assert q(1, 0) == 0 and q(0, 64) == 0 and q(-1, 64) == 0 and q(4, -1) == 0
    assert q(1, 16385) == 0 and q(65536, 8) == 0
    for B, N in ((1, 1), (3, 37), (32, 640), (1, 16384)):
        assert q(B, N) >= 8 * B * N + 4 * B + 4  # a vector per instance, a stop flag per instance, one word


def test_abi_argument_errors_return_before_any_device_work(lib):
    dev = 1 << 20  # never dereferenced
    ws = lib.lapwarm_ragged_duals_workspace_bytes(3, 300)
    head = dict(C=dev, offsets=dev, sizes=dev, ld=0, batch=3, N=300)
    tail = dict(ws=dev, ws_bytes=ws, stream=None)

    def rowmin(**c):
        a = dict(head, v=None, out=dev, ret=None, **tail)
        a.update(c)
        return lib.lapwarm_rowmin_ragged(a["C"], a["offsets"], a["sizes"], a["ld"], a["batch"], a["N"], a["v"],
                                         a["out"], a["ret"], a["ws"], a["ws_bytes"], a["stream"])

    def project(**c):
        a = dict(head, u=dev, v=dev, max_rounds=50, tol=1e-12, gmin=dev, rounds=dev, ret=dev, **tail)
        a.update(c)
        return lib.lapwarm_project_feasible_ragged(a["C"], a["offsets"], a["sizes"], a["ld"], a["batch"], a["N"],
                                                   a["u"], a["v"], a["max_rounds"], a["tol"], a["gmin"],
                                                   a["rounds"], a["ret"], a["ws"], a["ws_bytes"], a["stream"])

    def reduce(**c):
        a = dict(head, u=dev, v=dev, shift=1, out=None, gmin=dev, ret=None, **tail)
        a.update(c)
        return lib.lapwarm_reduce_costs_ragged(a["C"], a["offsets"], a["sizes"], a["ld"], a["batch"], a["N"],
                                               a["u"], a["v"], a["shift"], a["out"], a["gmin"], a["ret"], a["ws"],
                                               a["ws_bytes"], a["stream"])

    for call in (rowmin, project, reduce):
        assert call(N=0) == -2 and call(batch=0) == -2 and call(batch=65536) == -2 and call(ld=-1) == -2
        assert call(C=None) == -2 and call(offsets=None) == -2 and call(sizes=None) == -2 and call(ws=None) == -2
        assert call(N=16385) == -5
        assert call(ws_bytes=ws - 1) == -1
    assert rowmin(out=None) == -2
    for name in ("u", "v", "gmin", "rounds", "ret"):
        assert project(**{name: None}) == -2, name
    for name in ("u", "v", "gmin"):
        assert reduce(**{name: None}) == -2, name


# ------------------------------------------------------------------------------------------- the fixture
def test_fixture_is_no_larger_than_the_largest_one_and_holds_every_case():
    from dual_seeds_common import FIXTURE
    others = [p.stat().st_size for p in FIXTURE.parent.glob("*.npz") if p != FIXTURE]
    assert FIXTURE.stat().st_size <= max(others) and FIXTURE.stat().st_size <= 1 << 20
    z = cases()
    assert z["sizes"].tolist() == [1, 2, 7, 33, 64, 65]
    assert z["max_rounds"].tolist() == [0, 1, 3] and z["tols"].tolist() == [1e-12, -1e-3, -0.5]
    for kind, n, seed in case_names():
        key = case_key(kind, n, seed)
        assert z[f"rounds__{key}"].shape == (3, 3) and f"u0__{key}" in z.files
    n_inf = [int(np.isinf(matrix("inf", n)).sum()) for n in (7, 33, 64, 65)]
    assert all(k >= 2 for k in n_inf) and np.isneginf(matrix("inf", 33)).sum() == 1
    assert all(np.isnan(matrix("nan", int(n))).sum() == 1 for n in z["sizes"])
    C = matrix("int", 33)
    assert (C == np.round(C)).all() and len(np.unique(C)) == 5  # ties everywhere


@quiet_warnings
def test_numpy_statements_reproduce_the_fixture_and_the_two_read_gmin_is_the_three_read_one():
    z = cases()
    for kind, n, seed in case_names():
        key, C = case_key(kind, n, seed), matrix(kind, n)
        u0, v0 = z[f"u0__{key}"], z[f"v0__{key}"]
        for a, b, mr, tol in combos():
            u, v, gmin, rounds = np_project(C, u0, v0, mr, tol)
            u2, v2, gmin2, rounds2 = np_project(C, u0, v0, mr, tol, two_read=True)
            r = int(z[f"rounds__{key}"][a, b])
            assert rounds == r and rounds2 == r, (key, mr, tol)
            assert same(u, z[f"u__{key}__r{r}"]) and same(v, z[f"v__{key}__r{r}"]), (key, mr, tol)
            assert same(gmin, z[f"gmin__{key}__r{r}"]) and same(gmin2, gmin), (key, mr, tol)
            assert same(u2, u) and same(v2, v)
        feasible = not np_reduce(C, u0, v0, False)[1] < -1e-8
        assert feasible == bool(z[f"feasible__{key}"]), key
    for key in [str(k) for k in z["reduced_cases"]]:
        kind, nn, seed = key.split("_")
        C = matrix(kind, int(nn[1:]))
        assert same(np_reduce(C, z[f"u0__{key}"], z[f"v0__{key}"], True)[0], z[f"red_shift__{key}"]), key
        if f"red_noshift__{key}" in z.files:
            assert same(np_reduce(C, z[f"u0__{key}"], z[f"v0__{key}"], False)[0], z[f"red_noshift__{key}"]), key
    for kind in z["kinds"]:
        for n in z["sizes"]:
            u, v = np_seed_row_col_minima(matrix(str(kind), int(n)))
            assert same(u, z[f"rcseed_u__{kind}_n{n}"]) and same(v, z[f"rcseed_v__{kind}_n{n}"])


@quiet_warnings
def test_two_read_gmin_on_random_tied_infinite_and_nan_rounds():
    """min_i fl(fl(C_ij - u_i) - v_j) = fl(cap_j - v_j) round by round, also where infinities meet."""
    rs = np.random.RandomState(5)
    specials = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e308, -1e308])
    for trial in range(300):
        n = int(rs.randint(1, 9))
        C = rs.randint(0, 4, (n, n)).astype(np.float64) if trial % 2 else rs.uniform(-1, 1, (n, n))
        u, v = rs.uniform(-1, 1, n), rs.uniform(-1, 1, n)
        for arr in (C.reshape(-1), u, v):
            hit = rs.uniform(size=arr.shape) < (0.0, 0.1, 0.3)[trial % 3]
            arr[hit] = specials[rs.randint(0, len(specials), int(hit.sum()))]
        for _ in range(3):
            u = np.minimum(u, (C - v[None, :]).min(axis=1))
            cap = (C - u[:, None]).min(axis=0)
            v = np.minimum(v, cap)
            assert same((cap - v).min(), ((C - u[:, None]) - v[None, :]).min()), (trial, C, u, v)


def test_stop_cases_finite_inputs_stop_after_one_round_with_the_default_tol():
    """On finite costs a round ends with gmin >= 0 exactly, so only tol < 0 or NaN gives a second round; seeds so
    low that no column is capped stop at round 1 even under tol = -0.5.  The fixture holds each kind."""
    z = cases()
    seen = set()
    for kind, n, seed in case_names():
        key = case_key(kind, n, seed)
        table = z[f"rounds__{key}"]
        assert (table[:2] == 1).all()  # max_rounds 0 and 1: one round
        if kind in ("uni", "int"):
            assert (table[:, 0] == 1).all(), key
            assert float(z[f"gmin__{key}__r1"]) >= 0.0, key
        if seed == "low" and kind in ("uni", "int"):
            assert (table == 1).all() and float(z[f"gmin__{key}__r1"]) >= 0.5, key
            seen.add("stops at round 1 under every tol")
        if kind == "nan" and n > 1:
            seen.add("NaN")
            assert (table[2] == 3).all() and np.isnan(z[f"gmin__{key}__r3"]), key
        if kind in ("uni", "int") and table[2, 0] == 1 and table[2, 2] == 3:
            seen.add("stops at round 1 or never, by tol")
    assert len(seen) == 3, seen


# ------------------------------------------------------------------------------------------- Python surface
def hand_pack(sizes=(2, 3), dtype=None):
    import torch
    from gnn.features import RaggedPack
    sq = [n * n for n in sizes]
    C = torch.zeros(sum(sq), dtype=dtype or torch.float64)
    offsets = torch.tensor(np.concatenate(([0], np.cumsum(sq)[:-1])), dtype=torch.int64)
    return RaggedPack(C, offsets, torch.tensor(sizes, dtype=torch.int32), None, None, 0, max(sizes), list(sizes))


def test_pipeline_entries_raise_argument_errors_without_a_device():
    import torch
    from gnn.pipeline import WarmStartPipeline
    pipe = object.__new__(WarmStartPipeline)  # no device: the checks come before anything that needs one
    pack = hand_pack()
    good = torch.zeros((2, 3), dtype=torch.float64)
    calls = {
        "project": lambda p, u, v: pipe.project_feasible_ragged(p, u, v),
        "reduce": lambda p, u, v: pipe.reduce_costs_ragged(p, u, v),
        "feasible": lambda p, u, v: pipe.dual_feasible_ragged(p, u, v),
        "noisy": lambda p, u, v: pipe.noisy_duals_ragged(p, u, v, 0.1),
    }
    for name, call in calls.items():
        with pytest.raises(TypeError, match="Argument 'pack' must be a RaggedPack"):
            call([np.zeros((2, 2))], good, good)
        with pytest.raises(TypeError, match="packed costs must be torch.float64"):
            call(hand_pack(dtype=torch.float32), good, good)
        with pytest.raises(TypeError, match="Argument 'u' must be a torch.Tensor, not ndarray"):
            call(pack, good.numpy(), good)
        with pytest.raises(TypeError, match="v must be torch.float64, not torch.float32"):
            call(pack, good, good.float())
        with pytest.raises(ValueError, match=r"u must be a contiguous \(2, 3\) tensor, not \(2, 4\)"):
            call(pack, torch.zeros((2, 4), dtype=torch.float64), good)
        with pytest.raises(ValueError, match=r"v must be a contiguous \(2, 3\) tensor"):
            call(pack, good, torch.zeros((3, 2), dtype=torch.float64).t())
    with pytest.raises(TypeError, match="Argument 'max_rounds' must be an int, not float"):
        pipe.project_feasible_ragged(pack, good, good, max_rounds=2.5)
    with pytest.raises(TypeError, match="Argument 'tol' must be a float, not str"):
        pipe.project_feasible_ragged(pack, good, good, tol="1e-8")
    with pytest.raises(TypeError, match="Argument 'tol' must be a float"):
        pipe.dual_feasible_ragged(pack, good, good, tol=None)
    with pytest.raises(TypeError, match="Argument 'pack' must be a RaggedPack"):
        pipe.seed_row_col_minima_ragged(np.zeros((2, 2)))
    with pytest.raises(TypeError, match="Argument 'project_rounds' must be an int, not bool"):
        pipe.seed_row_col_minima_ragged(pack, project_rounds=True)
    with pytest.raises(TypeError, match="Argument 'generator' must be a torch.Generator"):
        pipe.noisy_duals_ragged(pack, good, good, 0.1, generator=np.random.default_rng(0))
    with pytest.raises(ValueError, match="noise_std must be >= 0, not -0.1"):
        pipe.noisy_duals_ragged(pack, good, good, -0.1)
    with pytest.raises(ValueError, match=r"prob must be in \[0, 1\], not 1.5"):
        pipe.noisy_duals_ragged(pack, good, good, 0.1, prob=1.5)
    with pytest.raises(TypeError, match="Argument 'project_rounds' must be an int"):
        pipe.noisy_duals_ragged(pack, good, good, 0.1, project_rounds="75")
    with pytest.raises(ValueError, match=r"dual_noise_prob must be in \[0, 1\], not -0.5"):
        pipe.training_batch([np.zeros((2, 2))], dual_noise_std=0.1, dual_noise_prob=-0.5)
    with pytest.raises(ValueError, match="dual_noise_std must be >= 0, not nan"):
        pipe.training_batch([np.zeros((2, 2))], dual_noise_std=float("nan"), dual_noise_prob=0.5)
    with pytest.raises(TypeError, match="Argument 'generator' must be a torch.Generator"):
        pipe.training_batch([np.zeros((2, 2))], dual_noise_std=0.1, dual_noise_prob=0.5, generator=3)


def test_row_min_ragged_raises_argument_errors_without_a_device():
    import torch
    from gnn import row_min_ragged
    pack = hand_pack()
    with pytest.raises(TypeError, match="Argument 'pack' must be a RaggedPack"):
        row_min_ragged(np.zeros((2, 2)))
    with pytest.raises(TypeError, match="Argument 'v' must be a torch.Tensor, not list"):
        row_min_ragged(pack, [0.0])
    with pytest.raises(TypeError, match="v must be torch.float64, not torch.int64"):
        row_min_ragged(pack, torch.zeros((2, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"v must be a contiguous \(2, 3\) tensor, not \(3,\)"):
        row_min_ragged(pack, torch.zeros(3, dtype=torch.float64))


def test_many_functions_raise_argument_errors_without_a_device():
    import solvers
    C2, C3 = np.zeros((2, 2)), np.zeros((3, 3))
    z2, z3 = np.zeros(2), np.zeros(3)
    for fn in (solvers.project_feasible_many, solvers.reduce_costs_many, solvers.check_dual_feasible_many):
        with pytest.raises(ValueError, match="at least one cost matrix expected"):
            fn([], [], [])
        with pytest.raises(ValueError, match=r"square, non-empty cost matrices expected, not \(2, 3\)"):
            fn([np.zeros((2, 3))], [z2], [z2])
        with pytest.raises(ValueError, match="2 instances but 1 vectors in us"):
            fn([C2, C3], [z2], [z2, z3])
        with pytest.raises(ValueError, match=r"vs\[1\] has shape \(2,\) for an instance of size 3"):
            fn([C2, C3], [z2, z3], [z2, z2])
    for fn in (solvers.seed_row_col_minima_many, solvers.seed_noisy_optimal_many):
        with pytest.raises(ValueError, match="at least one cost matrix expected"):
            fn([])
        with pytest.raises(ValueError, match=r"square, non-empty cost matrices expected, not \(0, 0\)"):
            fn([np.zeros((0, 0))])


def test_new_names_are_exported_and_training_batch_keeps_its_defaults():
    import gnn
    import solvers
    from gnn.pipeline import WarmStartPipeline
    from solvers import advanced_dual, seed_baselines
    for name in ("project_feasible_many", "reduce_costs_many", "check_dual_feasible_many"):
        assert name in advanced_dual.__all__ and name in solvers.__all__
    for name in ("seed_row_col_minima_many", "seed_noisy_optimal_many"):
        assert name in seed_baselines.__all__ and name in solvers.__all__
    assert "row_min_ragged" in gnn.__all__
    p = inspect.signature(WarmStartPipeline.training_batch).parameters
    assert list(p) == ["self", "costs", "dual_noise_std", "dual_noise_prob", "generator"]
    assert p["costs"].default is inspect.Parameter.empty
    assert (p["dual_noise_std"].default, p["dual_noise_prob"].default, p["generator"].default) == (0.0, 0.0, None)
    assert inspect.signature(WarmStartPipeline.project_feasible_ragged).parameters["max_rounds"].default == 50
    assert inspect.signature(WarmStartPipeline.noisy_duals_ragged).parameters["project_rounds"].default == 75
    assert inspect.signature(solvers.seed_noisy_optimal_many).parameters["noise_std"].default == 0.05
