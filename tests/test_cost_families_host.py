"""The device generator of the synthetic cost families without a GPU: the workspace query, the argument errors of the
three C entries (returned before the first HIP call), the host-side validation of gnn.synthetic, and the conditions on
the NumPy restatement (cost_families_common.py) that the GPU tests rest on: the ranges and moments of the draws, and
that the seeds of the GPU cases reach the repairs, both clamp branches and shared bins."""
import inspect

import numpy as np
import pytest

import cost_families_common as cf
from host_common import lib  # noqa: F401


def test_workspace_query_is_zero_out_of_range_and_grows_with_the_batch(lib):
    q = lib.lapwarm_cost_families_workspace_bytes
    assert q(1, 0) == 0 and q(0, 64) == 0 and q(-1, 64) == 0 and q(4, -1) == 0
    assert q(1, 16385) == 0 and q(65536, 8) == 0
    grid_b, grid_n = (1, 2, 3, 31, 32, 65535), (1, 7, 8, 9, 129, 640, 16384)
    for a, B in enumerate(grid_b):
        for k, N in enumerate(grid_n):
            assert q(B, N) >= 2 * 8 * B * N * 64 + 8 * B * ((N + 7) // 8) + B * N  # factors, tile minima, flags
            if a:
                assert q(B, N) >= q(grid_b[a - 1], N)
            if k:
                assert q(B, N) >= q(B, grid_n[k - 1])


def test_abi_argument_errors_return_before_any_device_work(lib):
    from lap import _hip
    dev = 1 << 20  # never dereferenced
    ws = lib.lapwarm_cost_families_workspace_bytes(3, 300)
    good = dict(C=dev, offsets=dev, sizes=dev, ld=0, batch=3, N=300, family=dev, seeds=dev, params=dev, ret=dev,
                ws=dev, ws_bytes=ws, stream=None)

    def call(**c):
        a = dict(good)
        a.update(c)
        return lib.lapwarm_generate_costs_ragged(*[a[k] for k in good])

    assert call(N=0) == -2 and call(batch=0) == -2 and call(batch=65536) == -2 and call(ld=-1) == -2
    for name in ("C", "offsets", "sizes", "family", "seeds", "params", "ret", "ws"):
        assert call(**{name: None}) == -2, name
    assert call(N=16385) == -5
    assert call(ws_bytes=ws - 1) == -1
    assert _hip.last_error().startswith("workspace too small")
    assert call(ws_bytes=0) == -1
    # the check order of the ragged entries: dimensions, then pointers, then the workspace
    assert call(N=0, C=None) == -2 and call(N=16385, C=None) == -5 and call(C=None, ws_bytes=0) == -2

    draws = lib.lapwarm_cost_family_draws
    assert draws(1, 0, 3, 0, 4, 1, dev, None) == -2 and draws(1, 0, -1, 0, 4, 1, dev, None) == -2
    assert draws(1, 0, 2, 0, 4, 0, dev, None) == -2 and draws(1, 0, 2, 0, 4, 2**31, dev, None) == -2
    assert draws(1, 0, 0, 0, 4, 0, None, None) == -2 and draws(1, 0, 0, 0, 1 << 39, 0, dev, None) == -2
    assert draws(1, 0, 0, 0, 0, 0, None, None) == 0  # nothing to draw


def test_synthetic_pack_validates_on_the_host(monkeypatch):
    from gnn import synthetic
    from lap import _hip

    def no_device():
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(_hip, "require_device", no_device)
    ok = (["uniform", "sparse"], [4, 5], [1, 2])
    with pytest.raises(AssertionError, match="the device was touched"):
        synthetic.synthetic_pack(*ok)  # the valid call is the one that reaches the device
    with pytest.raises(KeyError, match="Unknown family 'unifrom'"):
        synthetic.synthetic_pack(["unifrom", "sparse"], [4, 5], [1, 2])
    with pytest.raises(ValueError, match="2 families but 1 sizes and 2 seeds"):
        synthetic.synthetic_pack(["uniform", "sparse"], [4], [1, 2])
    with pytest.raises(ValueError, match="2 families but 2 sizes and 3 seeds"):
        synthetic.synthetic_pack(["uniform", "sparse"], [4, 5], [1, 2, 3])
    with pytest.raises(ValueError, match="2 families but 1 parameter sets"):
        synthetic.synthetic_pack(*ok, params=[None])
    with pytest.raises(ValueError, match="at least one instance"):
        synthetic.synthetic_pack([], [], [])
    with pytest.raises(ValueError, match="instance 1: n must be an integer >= 1, not 0"):
        synthetic.synthetic_pack(["uniform", "sparse"], [4, 0], [1, 2])
    with pytest.raises(ValueError, match="n must be an integer >= 1, not 4.0"):
        synthetic.synthetic_pack(["uniform"], [4.0], [1])
    with pytest.raises(ValueError, match="n exceeds the 16384 limit"):
        synthetic.synthetic_pack(["uniform"], [16385], [1])
    with pytest.raises(ValueError, match="rank must be in 1..64, not 65"):
        synthetic.synthetic_pack(["low_rank"], [4], [1], params=[{"rank": 65}])
    with pytest.raises(ValueError, match="rank must be in 1..64, not 0"):
        synthetic.synthetic_pack(["noisy_linear"], [4], [1], params=[{"rank": 0}])
    with pytest.raises(ValueError, match="blocks must be an integer, not 2.5"):
        synthetic.synthetic_pack(["clustered"], [4], [1], params=[{"blocks": 2.5}])
    with pytest.raises(ValueError, match="sparsity must be a finite number"):
        synthetic.synthetic_pack(["sparse"], [4], [1], params=[{"sparsity": float("nan")}])
    with pytest.raises(ValueError, match="tie has no parameter 'rank'"):
        synthetic.synthetic_pack(["tie"], [4], [1], params=[{"rank": 3}])
    for seed in (-1, 2**64, 1.5, None):
        with pytest.raises(ValueError, match="the seed must be an integer in 0..2\\^64-1"):
            synthetic.synthetic_pack(["uniform"], [4], [seed])
    with pytest.raises(ValueError, match="at most 65535 instances"):
        synthetic.synthetic_pack(["uniform"] * 65536, [1] * 65536, [0] * 65536)


def test_names_defaults_and_signatures():
    import gnn
    from gnn import synthetic
    from gnn.pipeline import DualWarmStartPipeline, WarmStartPipeline
    from solvers import generators
    for name in ("FAMILY_IDS", "DEFAULT_PARAMS", "synthetic_pack", "SyntheticStream"):
        assert name in gnn.__all__ and getattr(gnn, name) is getattr(synthetic, name)
    assert gnn.FAMILY_IDS == dict(cf.FAMILY_IDS, block=3)
    assert gnn.DEFAULT_PARAMS == {"uniform": {}, "metric": {}, "low_rank": {"rank": 12, "sigma": 0.1},
                                  "clustered": {"blocks": 4, "noise": 0.1}, "block": {"blocks": 4, "noise": 0.1},
                                  "noisy_linear": {"rank": 1, "noise": 0.1}, "tie": {"bins": 5, "jitter": 1e-6},
                                  "sparse": {"sparsity": 0.3}}
    assert set(gnn.FAMILY_IDS) == set(generators.FAMILIES)
    p = inspect.signature(synthetic.synthetic_pack).parameters
    assert list(p) == ["families", "sizes", "seeds", "device", "params", "padded"]
    assert (p["device"].default, p["params"].default, p["padded"].default) == ("cuda:0", None, False)
    for method in (WarmStartPipeline.synthetic_training_batch, DualWarmStartPipeline.synthetic_dual_training_batch):
        p = inspect.signature(method).parameters
        assert list(p) == ["self", "families", "sizes", "seeds", "params", "dual_noise_std", "dual_noise_prob",
                           "generator"]
        assert (p["params"].default, p["dual_noise_std"].default, p["dual_noise_prob"].default,
                p["generator"].default) == (None, 0.0, 0.0, None)
    assert "NOT the same matrices" in generators.generate_family_device.__doc__
    with pytest.raises(KeyError, match="Unknown family"):
        generators.generate_family_device("nope", 4, 0)


def test_training_batch_arguments_are_checked_before_any_device_work():
    from gnn import OneGNN
    from gnn.pipeline import WarmStartPipeline
    pipe = object.__new__(WarmStartPipeline)
    pipe.model = OneGNN(21, hidden=8, layers=1)
    with pytest.raises(ValueError, match=r"dual_noise_prob must be in \[0, 1\], not 2"):
        pipe.synthetic_training_batch(["uniform"], [4], [0], dual_noise_std=0.1, dual_noise_prob=2)
    with pytest.raises(TypeError, match="synthetic_dual_training_batch needs a pipeline around a DualGNN"):
        pipe.synthetic_dual_training_batch(["uniform"], [4], [0])
    with pytest.raises(TypeError, match="dual_training_batch needs a pipeline around a DualGNN"):
        pipe.dual_training_batch([np.zeros((2, 2))])


def test_stream_repeats_its_plans_and_draws_from_what_it_was_given():
    from gnn import SyntheticStream
    fams, sizes = ("uniform", "sparse", "metric", "clustered"), (5, 9, 33)
    a, b, c = SyntheticStream(fams, sizes, 6, 11), SyntheticStream(fams, sizes, 6, 11), SyntheticStream(fams, sizes, 6, 12)
    assert iter(a) is a
    plans = [next(a) for _ in range(3)]
    assert plans == [next(b) for _ in range(3)] and plans[0] != plans[1] and plans[0] != next(c)
    for f, s, seeds in plans:
        assert len(f) == len(s) == len(seeds) == 6 and set(f) <= set(fams) and set(s) <= set(sizes)
        assert all(isinstance(x, int) and 0 <= x < 2**64 for x in seeds)
    assert any(x >= 2**63 for _, _, seeds in plans for x in seeds)  # the whole 64 bits
    with pytest.raises(KeyError):
        SyntheticStream(("nope",), sizes, 2, 0)
    with pytest.raises(ValueError):
        SyntheticStream(fams, (0,), 2, 0)


# ------------------------------------------------------------------------------------------- the restatement
def test_uniforms_and_integers_are_in_range_and_one_draw_is_a_function_of_its_element():
    seed = cf.SEED_DRAWS
    u = cf.uniforms(seed, 0, 0, 1 << 16)
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 5 / np.sqrt(12 * u.size)
    assert cf.dbl(np.uint64(2**32 - 1), np.uint64(2**32 - 1)) == 1.0 - 2.0**-53 and cf.dbl(np.uint64(0), np.uint64(63)) == 0
    for m in (1, 5, 7, 2**31 - 1):
        i = cf.integers(seed, 4, 0, 4099, m)
        assert i.min() >= 0 and i.max() < m
    # a range read from the middle is the same draws: no state
    assert np.array_equal(cf.uniforms(seed, 0, 1001, 77), cf.uniforms(seed, 0, 0, 2000)[1001:1078])
    assert np.array_equal(cf.integers(seed, 5, 1001, 77, 9), cf.integers(seed, 5, 0, 2000, 9)[1001:1078])
    assert np.array_equal(cf.normals_numpy(seed, 1, 1001, 77), cf.normals_numpy(seed, 1, 0, 2000)[1001:1078])
    assert not np.array_equal(cf.uniforms(seed, 0, 0, 64), cf.uniforms(seed, 4, 0, 64))
    assert not np.array_equal(cf.uniforms(seed, 0, 0, 64), cf.uniforms(seed ^ (1 << 63), 0, 0, 64))


def test_normals_have_the_moments_of_a_standard_normal():
    N = 1 << 18
    z = cf.normals_numpy(cf.SEED_DRAWS, 1, 0, N)
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 5 / np.sqrt(N) and abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / N)
    ref = cf.normals_reference(cf.SEED_DRAWS, 1, cf.DRAWS_FIRST, cf.DRAWS_COUNT)
    assert np.abs(ref - cf.normals_numpy(cf.SEED_DRAWS, 1, cf.DRAWS_FIRST, cf.DRAWS_COUNT)).max() < 1e-14


def test_sparse_seeds_reach_a_row_repair_and_a_column_repair_after_it():
    assert all(3 <= n <= 8 for n in cf.SPARSE_SEEDS)
    for n, seed in cf.SPARSE_SEEDS.items():
        assert seed == cf.search_sparse_seed(n)  # the first seed that does
        keep, rows, cols = cf.sparse_keep(n, seed, 0.3)
        assert len(rows) >= 1 and len(cols) >= 1
        row_entries = {(i, int(cf.integers(seed, cf.REPAIR, i, 1, n)[0])) for i in rows}
        col_entries = {(int(cf.integers(seed, cf.REPAIR, n + j, 1, n)[0]), j) for j in cols}
        assert col_entries - row_entries, (n, seed)  # a column repair that is not also a row's
        assert keep.any(axis=0).all() and keep.any(axis=1).all()
        C = cf.matrix("sparse", n, seed)
        assert ((C < 1.0) == keep).all() and (C[~keep] == 1e6).all()
    used = {(n, seed) for family, n, seed, _, _ in cf.cases() if family == "sparse"}
    assert {(n, s) for n, s in cf.SPARSE_SEEDS.items()} <= used


def test_case_seeds_reach_both_clamp_branches_and_shared_bins():
    seen = set()
    for family, n, seed, p0, p1 in cf.cases():
        C = cf.matrix(family, n, seed, p0, p1)
        assert C.shape == (n, n) and np.isfinite(C).all() and (C >= 0).all()
        if family in ("low_rank", "clustered") and n >= 7:
            # both branches, and no value so near 0 that another libm could change the branch
            assert (C == 0).any() and (C > 0).any(), (family, n)
            seen.add(family)
        if family == "tie" and n >= 3:
            m = max(1, p0)
            bins = cf.integers(seed, cf.MASK, 0, n * n, m).reshape(n, n)
            assert any(len(set(row)) < n for row in bins.tolist()), (n, seed)
            assert np.array_equal(np.floor(C * m + 0.5 * p1).astype(np.int64), bins)
            seen.add("tie")
        if family == "noisy_linear":
            assert C.min() == 0.0
        if family == "clustered" and p0 == 132:
            assert n + 3 == p0  # more blocks than rows: only the diagonal is in-cluster
    assert seen == {"low_rank", "clustered", "tie"}
    ranks = {p0 for family, _, _, p0, _ in cf.cases() if family == "low_rank"}
    blocks = {(p0, n) for family, n, _, p0, _ in cf.cases() if family == "clustered"}
    bins = {p0 for family, _, _, p0, _ in cf.cases() if family == "tie"}
    assert {1, 12, 64} <= ranks and {1, 5} <= bins and {(1, 9), (4, 9), (132, 129)} <= blocks


def test_mixed_batch_has_five_families_distinct_sizes_and_an_odd_size_before_another_instance():
    fams, sizes = [f for f, _, _ in cf.MIXED], [n for _, n, _ in cf.MIXED]
    live = [(f, n) for f, n in zip(fams, sizes) if n]
    assert len(live) == 5 and len({f for f, _ in live}) == 5 and len({n for _, n in live}) == 5 and sizes.count(0) == 1
    offsets = np.concatenate(([0], np.cumsum(np.asarray(sizes) ** 2)))[:-1]
    assert any(n and o % 2 == 1 for n, o in zip(sizes, offsets))  # 8 bytes off a 16-byte boundary
