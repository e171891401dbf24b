"""The references and builders of tests/dense_sweeps_common.py, checked on the CPU against what the
project already trusts: oracle/features_np.py and OneGNN's reference-order refinement."""
import numpy as np
import pytest

import dense_sweeps_common as dsc
from oracle import features_np


def test_colmin_chunks_give_the_chunk_shapes_the_sizes_were_chosen_for():
    assert dsc.colmin_chunks(2, 2048) == 1
    for n, last in ((993, 1), (1025, 1), (994, 2)):
        per = dsc.rows_per_chunk(n, 1)
        assert n - (dsc.colmin_chunks(n, 1) - 1) * per == last, n
    assert [n % 2 for n in (513, 1023, 993, 1025)] == [1, 1, 1, 1]
    assert 514 - 512 == 2  # second column tile of the pair path: one pair


@pytest.mark.parametrize("family", dsc.FINITE_FAMILIES)
def test_builders_plant_the_extrema_they_name(family):
    for B, n in ((3, 257), (2, 514), (1, 993), (5, 33), (3, 2), (1, 1)):
        base = dsc.costs(family, B, n)
        assert all(not np.array_equal(base[a], base[b]) for a in range(B) for b in range(a)) or n == 1
        C, cols = dsc.plant_row_minima(base)
        hit = cols >= 0
        assert np.array_equal(C.argmin(axis=2)[hit], cols[hit])
        two = np.sort(C, axis=2)[:, :, :2]
        assert n == 1 or (two[:, :, 1] > two[:, :, 0])[hit].all()  # strict
        assert set(np.unique(cols[hit])) == set(dsc.row_plant_columns(n))
        C, rows = dsc.plant_col_minima(base)
        hit = rows >= 0
        assert np.array_equal(C.argmin(axis=1)[hit], rows[hit])
        assert set(np.unique(rows[hit])) == set(dsc.col_plant_rows(n, B))
        assert len({C[b].min() for b in range(B)}) == B  # the plants differ between instances


def test_project_round_iterated_is_project_feasible():
    for family in dsc.FAMILIES:
        for B, n in ((3, 2), (5, 33), (3, 257)):
            C = dsc.planted(family, B, n)
            u0, v0 = dsc.project_seeds(C, feasible=(B - 1,))
            for b in range(B):
                with np.errstate(invalid="ignore"):
                    want = features_np.project_feasible(C[b], u0[b], v0[b], max_rounds=7)
                u, v = u0[b:b + 1], v0[b:b + 1]
                for _ in range(7):
                    u, v, g = dsc.project_round(C[b:b + 1], u, v)
                    if g[0] >= -1e-12:
                        break
                assert dsc.same(u[0], want[0]) and dsc.same(v[0], want[1]), (family, B, n, b)
            # the batched call is the per-instance call
            ub, vb, gb = dsc.project_round(C, u0, v0)
            for b in range(B):
                u1, v1, g1 = dsc.project_round(C[b], u0[b], v0[b])
                assert dsc.same(ub[b], u1) and dsc.same(vb[b], v1) and dsc.same(gb[b], g1)


def test_project_seeds_hold_a_feasible_instance_and_rounds_end_feasible():
    """A feasible instance is left as it is.  Every other finite instance is feasible after ONE round, with
    gmin >= 0 exactly and not just to a tolerance: v' <= fl(C - u') entry by entry, and fl(a - b) >= 0 for
    b <= a.  So no finite seed has gmin < 0 after a round; a negative global minimum reaches the same two
    kernels through reduce_costs (test_reduce_seeds_... below)."""
    for B, n in dsc.SHAPES:
        for family in dsc.FINITE_FAMILIES:
            C = dsc.planted(family, B, n)
            u0, v0 = dsc.project_seeds(C, feasible=(B - 1,))
            u1, v1, g1 = dsc.project_round(C, u0, v0)
            assert np.array_equal(u1[B - 1], u0[B - 1]) and np.array_equal(v1[B - 1], v0[B - 1])
            assert (g1 >= 0).all(), (family, B, n, g1)
            if B > 1 and n >= 33:
                assert not np.array_equal(u1[0], u0[0]) and not np.array_equal(v1[0], v0[0]), (family, B, n)
                raw, g0 = dsc.reduce_costs(C, u0, v0, False)
                assert (g0[:B - 1] < 0).all(), (family, B, n)  # the seeds themselves are infeasible


@pytest.mark.parametrize("family", dsc.FINITE_FAMILIES)
def test_reduce_seeds_give_a_negative_a_zero_and_a_positive_minimum(family):
    for B, n in ((3, 257), (1, 33), (2, 2), (1, 1)):
        C = dsc.planted(family, B, n)
        seen = set()
        for shift in range(3):
            u, v, kinds = dsc.reduce_seeds(C, shift)
            out, g = dsc.reduce_costs(C, u, v, True)
            raw, _ = dsc.reduce_costs(C, u, v, False)
            for b, kind in enumerate(kinds):
                assert {"negative": g[b] < 0, "zero": g[b] == 0, "positive": g[b] > 0}[kind], (n, b, kind, g[b])
                assert np.array_equal(out[b], raw[b] - g[b] if kind == "negative" else raw[b])
                seen.add(kind)
        assert seen == set(dsc.REDUCE_KINDS)


def _prenorm_message(model, top, u_pre, mask):
    """OneGNN._refine_reference_order without its final LayerNorm, in the model's dtype."""
    import torch
    from torch import nn
    norm = model.message_norm
    model.message_norm = nn.Identity()
    try:
        with torch.no_grad():
            h = torch.zeros(top.shape[:2] + (model.pre_out.in_features,), dtype=top.dtype)
            return model._refine_reference_order(h, top, u_pre, None if mask is None else mask.unsqueeze(-1))
    finally:
        model.message_norm = norm


@pytest.mark.parametrize("H", [2, 3, 64])
def test_refine_aggregate_ref_then_second_layer_is_the_reference_order_message(H):
    import torch
    from gnn import OneGNN
    torch.manual_seed(H)
    model = OneGNN(21, hidden=H, layers=1).eval().double()
    lin1, lin2 = model.edge_mlp[0], model.edge_mlp[2]
    w1 = lin1.weight.detach().view(-1).numpy()
    b1 = lin1.bias.detach().numpy()
    B, N = 2, 40
    seen = set()
    for shift in range(3):
        top, u_pre, kinds = dsc.refine_inputs(B * N, seed=H, shift=shift, grid=True)
        seen |= set(kinds)
        mask = torch.ones((B, N), dtype=torch.bool)
        mask[0, 3] = mask[1, 7] = mask[1, N - 1] = False
        want = _prenorm_message(model, torch.from_numpy(top).double().view(B, N, 16),
                                torch.from_numpy(u_pre).double().view(B, N), mask).numpy().reshape(B * N, H)
        masked = np.where(mask.numpy().reshape(-1, 1), top, np.float32(np.inf))  # as OneGNN._refine_fused
        agg, wsum = dsc.refine_aggregate_ref(masked, u_pre, w1, b1)
        got = agg @ lin2.weight.detach().numpy().T + wsum[:, None] * lin2.bias.detach().numpy()[None, :]
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (H, shift)
        dead = ~np.isfinite(masked - u_pre[:, None]).any(axis=1)
        assert dead.sum() >= 3 + kinds.count("masked") and (agg[dead] == 0).all() and (wsum[dead] == 0).all()
        assert np.abs(wsum[~dead] - 1.0).max() <= 1e-15
        ties = np.array([k == "ties" for k in kinds]) & ~dead
        x = (top[ties, 0] - u_pre[ties]).astype(np.float64)[:, None] * w1[None, :] + b1[None, :]
        xt = torch.from_numpy(x)
        assert np.allclose(agg[ties], (0.5 * xt * (1 + torch.erf(xt / 2 ** 0.5))).numpy(), rtol=1e-14, atol=1e-15)
    assert seen == set(dsc.REFINE_KINDS)


def test_refine_float32_yardstick_is_close_to_the_float64_reference():
    top, u_pre, _ = dsc.refine_inputs(64, seed=1)
    w1, b1 = dsc.refine_weights(192, seed=1)
    ref, wref = dsc.refine_aggregate_ref(top, u_pre, w1, b1)
    f32, w32 = dsc.refine_aggregate_f32(top, u_pre, w1, b1)
    assert f32.dtype == np.float32 and 0 < np.abs(f32 - ref).max() < 1e-5
    assert np.abs(w32 - wref).max() < 1e-6
