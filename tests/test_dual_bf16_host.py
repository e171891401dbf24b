"""The fused_edge_precision switch of DualGNN, the header's two bf16 entries, and the restatement of the bf16 contract
against itself (dual_bf16_common): the fp32 stand-in with a permuted summation order meets, with room, the criteria the
GPU tests put to the kernels, so the inputs suit the criteria.  No GPU."""
import re

import pytest
import torch

import dual_bf16_common as bc
from conftest import ROOT

NEW_SYMBOLS = ("lapwarm_dual_edge_scores_bf16", "lapwarm_dual_edge_scores_backward_bf16")


def test_the_switch_exists_and_defaults_to_fp32():
    from gnn.dual_gnn import DualGNN, DualLayer
    assert DualLayer.fused_edge_precision == "fp32"
    assert DualLayer(32, heads=4).fused_edge_precision == "fp32"
    assert DualGNN(hidden_dim=32, layers=2, heads=4).fused_edge_precision == "fp32"


def test_a_bad_value_raises_value_error():
    from gnn.dual_gnn import DualGNN, _edge_precision
    model = DualGNN(hidden_dim=32, layers=2, heads=4)
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(ValueError):
            model.fused_edge_precision = bad
        with pytest.raises(ValueError):
            _edge_precision(bad)
    assert model.fused_edge_precision == "fp32" and all(l.fused_edge_precision == "fp32" for l in model.layers)


def test_the_model_property_sets_every_layer():
    from gnn.dual_gnn import DualGNN
    model = DualGNN(hidden_dim=32, layers=3, heads=4)
    model.fused_edge_precision = "bf16"
    assert [layer.fused_edge_precision for layer in model.layers] == ["bf16"] * 3
    assert model.fused_edge_precision == "bf16"
    model.layers[1].fused_edge_precision = "fp32"
    assert model.fused_edge_precision == "fp32"   # not all layers
    model.fused_edge_precision = "fp32"
    assert [layer.fused_edge_precision for layer in model.layers] == ["fp32"] * 3


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_the_header_declares_the_bf16_entries(name):
    from lap import _hip
    header = (ROOT / "include" / "lapwarm_hip.h").read_text()
    m = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, name
    twin = name.replace("_backward_bf16", "_backward_dropout").replace("scores_bf16", "scores_dropout")
    assert len(m.group(1).split(",")) == len(_hip.SIGNATURES[name][1]) == len(_hip.SIGNATURES[twin][1])
    assert _hip.SIGNATURES[name] == _hip.SIGNATURES[twin]


@pytest.mark.parametrize("heads", [1, 4, 8])
def test_the_stand_in_meets_the_forward_criteria_with_room(heads):
    """E = 20 000 edges: the share of scores further than 1e-5 from the fp64 restatement is at most 0.4 % and the
    maximum difference at most half the flip bound."""
    args = bc.inputs(2, 100, heads)
    want, h2_max, g_max = bc.edge_scores(*args, dtype=torch.float64, parts=True)
    stand_in = bc.edge_scores(*args, dtype=torch.float32, permute=torch.Generator().manual_seed(5))
    share, worst = bc.share_and_max(stand_in, want)
    bound = bc.flip_bound(h2_max, g_max)
    print(f"heads={heads}: share {share:.5f}, max {worst:.3e}, flip bound {bound:.3e}")
    assert share <= 0.004
    assert worst <= 0.5 * bound


def test_straight_through_rounding_keeps_the_values_and_passes_the_gradient():
    args = bc.inputs(1, 5, 4)
    assert torch.equal(bc.edge_scores(*args, ste=True), bc.edge_scores(*args))
    grads = bc.edge_gradients(*args, torch.ones((1, 8, 5, 5)))
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in grads.values())
