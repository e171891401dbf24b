"""The float64 closed form of the refinement backward (tests/refine_backward_common.py) against torch float64
autograd of OneGNN._refine_reference_order, and the host-side pieces of the feature.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import dense_sweeps_common as dsc
import refine_backward_common as rbc

ROOT = Path(__file__).resolve().parents[1]

# (label, keyword arguments of refine_inputs, scale of refine_weights)
REGIMES = [("moderate", {}, 1.0), ("u_offset_1e3", {"u_offset": 1e3}, 1.0), ("weights_x50", {}, 50.0)]


def _model_grads(H, top, u_pre, w1, b1, Gm, second_layer):
    """float64 autograd of sum(Gm * message) through OneGNN._refine_reference_order without its LayerNorm, and
    without its second linear layer unless `second_layer`: grads of u_pre, edge_mlp[0].weight / .bias, and the
    (G, s) that reach the aggregate and the weight sum."""
    import torch
    from torch import nn
    from gnn import OneGNN
    torch.manual_seed(H)
    model = OneGNN(21, hidden=H, layers=1).eval().double()
    model.message_norm = nn.Identity()
    lin1 = model.edge_mlp[0]
    with torch.no_grad():
        lin1.weight.copy_(torch.from_numpy(w1).double().view(-1, 1))
        lin1.bias.copy_(torch.from_numpy(b1).double())
    Gm = torch.from_numpy(Gm).double()
    if second_layer:
        lin2 = model.edge_mlp[2]
        G = (Gm @ lin2.weight.detach()).numpy()
        s = (Gm @ lin2.bias.detach()).numpy()
    else:
        model.edge_mlp[2] = nn.Identity()
        G, s = Gm.numpy(), None
    rows = top.shape[0]
    up = torch.from_numpy(u_pre).double().view(1, rows).requires_grad_()
    base = torch.from_numpy(top).double().view(1, rows, dsc.K)
    h = torch.zeros((1, rows, H), dtype=torch.float64)
    msg = model._refine_reference_order(h, base, up, None)
    (Gm.view(1, rows, H) * msg).sum().backward()
    return (up.grad.view(-1).numpy(), lin1.weight.grad.view(-1).numpy(), lin1.bias.grad.numpy()), G, s


@pytest.mark.parametrize("second_layer", [False, True], ids=["G_only", "G_and_s"])
@pytest.mark.parametrize("regime", REGIMES, ids=[r[0] for r in REGIMES])
@pytest.mark.parametrize("rows,H", [(17, 3), (257, 192)])
def test_closed_form_is_float64_autograd_of_the_reference_order(rows, H, regime, second_layer):
    """All eight input kinds, none left out: the closed form agrees with autograd within 1e-12 of the largest
    gradient entry; so does the op-for-op restatement that the GPU tests use as their float32 yardstick.
    Inputs are on the 2**-10 grid, where float32 and float64 form the same topk - u_pre."""
    _, kw, scale = regime
    seen = set()
    for shift in (0, 3):
        top, u_pre, kinds = dsc.refine_inputs(rows, seed=H, shift=shift, grid=True, **kw)
        seen |= set(kinds)
        w1, b1 = dsc.refine_weights(H, seed=shift, scale=scale)
        Gm, _ = rbc.grad_seeds(rows, H, seed=shift)
        want, G, s = _model_grads(H, top, u_pre, w1, b1, Gm, second_layer)
        got = rbc.refine_backward_ref(top, u_pre, w1, b1, G, s)
        import torch
        restated = rbc.refine_autograd(top, u_pre, w1, b1, G, s, dtype=torch.float64)
        for name, a, b, c in zip(("grad_u", "grad_w1", "grad_b1"), got, want, restated):
            assert np.isfinite(b).all(), (name, shift)
            big = max(1.0, float(np.abs(b).max()))
            assert np.abs(a - b).max() <= 1e-12 * big, (name, shift, np.abs(a - b).max(), big)
            assert np.abs(c - b).max() <= 1e-12 * big, (name, shift, np.abs(c - b).max(), big)
        dead = np.array([k == "masked" for k in kinds])
        assert dead.any() or rows < 8
        assert (got[0][dead] == 0).all()
    assert seen == set(dsc.REFINE_KINDS)


def test_float32_yardstick_is_finite_on_every_kind():
    import torch
    for _, kw, scale in REGIMES:
        top, u_pre, kinds = dsc.refine_inputs(64, seed=5, **kw)
        assert set(kinds) == set(dsc.REFINE_KINDS)
        w1, b1 = dsc.refine_weights(192, seed=5, scale=scale)
        G, s = rbc.grad_seeds(64, 192)
        ref = rbc.refine_backward_ref(top, u_pre, w1, b1, G, s)
        f32 = rbc.refine_autograd(top, u_pre, w1, b1, G, s, dtype=torch.float32)
        for a, b in zip(f32, ref):
            assert a.dtype == np.float32 and np.isfinite(a).all() and np.isfinite(b).all()
            assert np.abs(a - b).max() <= 1e-3 * max(1.0, np.abs(b).max())


def test_wsum_gradient_cancels_where_the_weights_sum_to_one():
    """sum_k w_k = 1 on a live row, so s moves grad_u only by rounding: the closed form keeps the term, and
    the results with and without s agree to float64 rounding."""
    top, u_pre, _ = dsc.refine_inputs(40, seed=2)
    w1, b1 = dsc.refine_weights(8, seed=2)
    G, s = rbc.grad_seeds(40, 8)
    a = rbc.refine_backward_ref(top, u_pre, w1, b1, G, s)
    b = rbc.refine_backward_ref(top, u_pre, w1, b1, G, None)
    assert np.abs(a[0] - b[0]).max() <= 1e-13 * max(1.0, np.abs(b[0]).max())
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_fused_refine_training_is_a_plain_attribute():
    from gnn import OneGNN
    model = OneGNN(21, hidden=8, layers=1)
    assert model.fused_refine_training is False
    assert not any("fused_refine_training" in k for k in model.state_dict())
    model.fused_refine_training = True
    assert not any("fused_refine_training" in k for k in model.state_dict())
    assert OneGNN(21, hidden=8, layers=1).fused_refine_training is False
    with pytest.raises(TypeError):
        OneGNN(21, hidden=8, layers=1, fused_refine_training=True)


def test_cpu_training_path_is_the_reference_order_whatever_the_switch():
    import torch
    from gnn import OneGNN
    torch.manual_seed(0)
    model = OneGNN(21, hidden=8, layers=1, dropout=0.0).train()
    feat = torch.randn(2, 20, 21)
    topk = torch.sort(torch.rand(2, 20, 16), dim=-1).values
    u0 = model(feat, topk_values=topk)["u"]
    model.fused_refine_training = True
    assert torch.equal(model(feat, topk_values=topk)["u"], u0)


def test_abi_is_declared_and_bound():
    from lap import _hip
    header = (ROOT / "include" / "lapwarm_hip.h").read_text()
    for name in ("lapwarm_refine_backward_workspace_bytes", "lapwarm_refine_backward"):
        assert name in _hip.SIGNATURES
        assert re.search(r"\b%s\(" % name, header)
    assert len(_hip.SIGNATURES["lapwarm_refine_backward"][1]) == 14
