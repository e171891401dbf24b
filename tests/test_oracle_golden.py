"""The CPU checker (oracle/) against the golden vectors generated from the reference.

This is what pins the oracle: every fixture under tests/golden/ was produced by the
reference's own code (tests/golden/make_golden.py).  Integer results are compared
bit for bit; float32 features/duals within the tolerance written at each assert.
"""
import numpy as np
import pytest
import torch

from oracle import features_np, jv, one_gnn_ref


def test_seeded_solver_bit_exact(seeded_cases):
    branches = {}
    for k in range(len(seeded_cases)):
        c = seeded_cases.case(k)
        ret, x, y, st = jv.seeded_raw(c["C"], c["u"], c["v"], c["eps"])
        assert ret == c["ret"], c["label"]
        if ret == 0:
            assert np.array_equal(x, c["x"]), c["label"]
            assert np.array_equal(y, c["y"]), c["label"]
            branches[st["branch"]] = branches.get(st["branch"], 0) + 1
    # every branch of the seeded solve is represented in the fixtures
    assert set(branches) == {1, 2, 3}, branches


def test_seeded_fixtures_cover_projection_and_infeasible(seeded_cases):
    rets = [seeded_cases.case(k)["ret"] for k in range(len(seeded_cases))]
    assert -3 in rets
    fired = 0
    for k in range(len(seeded_cases)):
        c = seeded_cases.case(k)
        fired += jv.seeded_raw(c["C"], c["u"], c["v"], c["eps"])[3]["proj_events"] > 0
    assert fired > 20


def test_seeded_fixtures_cover_micro_arr_firing(seeded_cases):
    """lapjv_seeded.cpp:136-159 fires in >= 10 fixtures (x, y there come from the reference build)."""
    want = seeded_cases.z["arr_fired"]
    ks = [k for k in range(len(seeded_cases)) if want[k] > 0]
    assert len(ks) >= 10 and max(want) >= 2
    for k in ks:
        c = seeded_cases.case(k)
        ret, x, y, st = jv.seeded_raw(c["C"], c["u"], c["v"], c["eps"])
        assert ret == 0 and st["arr_fired"] == want[k] and st["branch"] == 1, c["label"]
        assert np.array_equal(x, c["x"]) and np.array_equal(y, c["y"]), c["label"]


def test_cold_solver_bit_exact(cold_cases):
    for k in range(len(cold_cases)):
        c = cold_cases.case(k)
        ret, x, y, _ = jv.dense_raw(c["C"])
        assert ret == c["ret"] == 0
        assert np.array_equal(x, c["x"]), c["label"]
        assert np.array_equal(y, c["y"]), c["label"]


def test_demo_cases_of_the_reference(seeded_cases):
    """LAP/test_seeded.py and LAP/demo_seeded.py print these; SURVEY 8(c) records them."""
    c = seeded_cases.case(seeded_cases.labels.index("demo3x3/zeros"))
    x, y, cost = jv.lapjv_seeded(c["C"], c["u"], c["v"])
    assert cost == 5.0 and list(x) == [1, 0, 2]
    c = seeded_cases.case(seeded_cases.labels.index("demo4x4/feasible"))
    x, y, cost = jv.lapjv_seeded(c["C"], c["u"], c["v"])
    assert cost == 8.0 and list(x) == [1, 2, 3, 0] and list(y) == [3, 0, 1, 2]


def test_row_features_match_reference(features_cases):
    z = features_cases
    assert tuple(z["empty_shape"]) == features_np.compute_row_features(np.zeros((0, 0))).shape
    assert int(z["row_feature_dim"]) == features_np.ROW_FEATURE_DIM == 21
    for key in [str(s) for s in z["labels"]]:
        got = features_np.compute_row_features(z[f"C__{key}"])
        want = z[f"feat__{key}"]
        assert got.dtype == np.float32 and got.shape == want.shape
        # float32 outputs of fp64 statistics: identical up to 1 ulp of summation order
        np.testing.assert_allclose(got, want, rtol=2e-7, atol=1e-12, err_msg=key)
        # counting features are exact
        assert np.array_equal(got[:, 11], want[:, 11]) and np.array_equal(got[:, 12], want[:, 12])


def test_dual_utilities_match_reference(features_cases):
    z = features_cases
    for key in [str(s) for s in z["labels"]]:
        C, u0, v0 = z[f"C__{key}"], z[f"u0__{key}"], z[f"v0__{key}"]
        pu, pv = features_np.project_feasible(C, u0, v0)
        assert np.array_equal(pu, z[f"proj_u__{key}"]) and np.array_equal(pv, z[f"proj_v__{key}"])
        if f"red_shift__{key}" in z.files:
            assert np.array_equal(features_np.reduce_costs(C, u0, v0, True), z[f"red_shift__{key}"])
            assert np.array_equal(features_np.reduce_costs(C, pu, pv, False), z[f"red_noshift__{key}"])


@pytest.mark.parametrize("tag", ["h64l2", "h192l4"])
def test_onegnn_forward_matches_reference(onegnn_cases, tag):
    z = onegnn_cases
    sd = {k.split("__", 2)[2]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"sd__{tag}__")}
    keys = [k[len("u__"):] for k in z.files if k.startswith(f"u__{tag}__") and not k.endswith("batch")]
    assert keys
    for key in keys:
        C = z[f"C__{key}"]
        u, v = one_gnn_ref.predict(sd, C)
        # same torch CPU kernels, same op order: tolerance is the north-star 1e-5
        np.testing.assert_allclose(u, z[f"u__{key}"], rtol=0, atol=1e-5, err_msg=key)
        np.testing.assert_allclose(v, z[f"v__{key}"], rtol=0, atol=1e-5, err_msg=key)
        feat = torch.from_numpy(features_np.compute_row_features(C)).float().unsqueeze(0)
        mask = torch.ones((1, C.shape[0]), dtype=torch.bool)
        u_nc = one_gnn_ref.forward(sd, feat, None, mask).squeeze(0).numpy()
        np.testing.assert_allclose(u_nc, z[f"u_nocost__{key}"], rtol=0, atol=1e-5, err_msg=key)
    if f"u__{tag}__batch" in z.files:
        Cb = z[f"C__{tag}__batch"]
        feat = torch.from_numpy(np.stack([features_np.compute_row_features(c) for c in Cb])).float()
        ub = one_gnn_ref.forward(sd, feat, torch.from_numpy(Cb).float(),
                                 torch.from_numpy(z[f"mask__{tag}__batch"])).numpy()
        np.testing.assert_allclose(ub, z[f"u__{tag}__batch"], rtol=0, atol=1e-5)


# --------------------------------------------------------------------------- the reference's lapjv suite
@pytest.fixture(scope="module")
def lapjv_suite():
    from lapjv_suite import Suite
    return Suite()


def test_reference_suite_integer_matrices_are_the_references(lapjv_suite):
    """solvers.generators.known_answer_int_costs rebuilds every integer matrix of test_lapjv.py (and the
    same recipe at n = 4608) bit for bit: sha256 of the fp64 matrix the reference's generator made."""
    from lapjv_suite import sha256
    assert len(lapjv_suite.int_labels) == 11
    for label in lapjv_suite.int_labels:
        C = lapjv_suite.matrix(label)
        assert sha256(C) == str(lapjv_suite.z[f"sha256__{label}"]), label
    spec = lapjv_suite.int_spec("s1k")
    assert spec["fill"] == float(np.iinfo(np.int64).max)
    assert (lapjv_suite.matrix("s1k") == spec["fill"]).sum() >= 1000  # a masked perfect matching at least


def test_reference_suite_regimes(lapjv_suite):
    """The suite reaches what the older fixtures do not: inf rows / columns, NaN (also in column 0),
    costs far above LARGE (1e6), n up to 4608."""
    s = lapjv_suite
    assert np.isinf(s.matrix("all_inf")).all() and np.isinf(s.matrix("inf_row")[2]).all()
    assert np.isinf(s.matrix("inf_col")[:, 1]).all()
    assert s.matrix("s4k").max() > 9e18 and s.matrix("s4k_i32").max() == 2147483647.0
    assert s.matrix("s4608").shape == (4608, 4608) and s.matrix("eps").shape == (368, 368)
    col0 = [k for k in s.nan_labels if k.endswith("_col0")]
    assert len(col0) == 6 and len(s.nan_labels) == 12
    for k in s.nan_labels:
        C = s.matrix(k)
        assert np.isnan(C).any()
        if k in col0:
            assert np.isnan(C[:, 0]).sum() > np.isnan(C[:, 1:]).sum(0).max(), k


def test_oracle_reproduces_reference_suite(lapjv_suite):
    """The oracle (cold and seeded) reproduces every output of the reference build on the suite, and
    the optima test_lapjv.py asserts: this pins the oracle on inf, NaN and 9.2e18 costs before the GPU
    tests judge the kernels against it."""
    from lapjv_suite import assert_known_optimum
    s = lapjv_suite
    n_seeded = 0
    for label in s.labels:
        C = s.matrix(label)
        ret, x, y, _ = jv.dense_raw(C)
        rr, rx, ry = s.cold(label)
        assert ret == rr == 0, label
        assert np.array_equal(x, rx) and np.array_equal(y, ry), label
        assert_known_optimum(s, label, C[np.arange(C.shape[0]), x].sum())
        if s.known_x(label) is not None:
            assert np.array_equal(x, s.known_x(label)), label
        for kind in s.seed_kinds(label):
            u, v = s.seeds(label, kind)
            ret, x, y, _ = jv.seeded_raw(C, u, v)
            rr, rx, ry = s.seeded(label, kind)
            assert ret == rr, (label, kind)
            if ret == 0:
                assert np.array_equal(x, rx) and np.array_equal(y, ry), (label, kind)
                assert_known_optimum(s, label, C[np.arange(C.shape[0]), x].sum())
            n_seeded += 1
    assert n_seeded >= len(s.labels) + 15
