"""DualGNN's fused dropout without a GPU: the NumPy restatement of the keep rule against the Random123 known answers,
the keep rate and the independence of the masks that the GPU tests draw, the switch and its routing, the header's
declarations and the argument codes of the new entries."""
import math
import re

import numpy as np
import pytest
import torch

import dual_dropout_common as ddc
import dual_gnn_common as dg
from conftest import ROOT
from host_common import lib  # noqa: F401
from lap import _hip

HEADER = (ROOT / "include" / "lapwarm_hip.h").read_text()
NEW_SYMBOLS = ("lapwarm_dual_edge_scores_dropout", "lapwarm_dual_attention_stats_dropout",
               "lapwarm_dual_attention_backward_dropout", "lapwarm_dual_edge_scores_backward_dropout",
               "lapwarm_dual_dropout_keep")

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, output
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_the_round_function_gives_the_random123_known_answers(counter, key, want):
    got = tuple(int(w) for w in ddc.philox4x32_10(counter, key))
    assert got == want, [hex(w) for w in got]


def test_one_round_is_the_stated_map():
    c, k = (1, 2, 3, 4), (5, 6)
    got = tuple(int(w) for w in ddc.philox_round(tuple(np.uint64(x) for x in c), tuple(np.uint64(x) for x in k)))
    p0, p1 = ddc.M0 * c[0], ddc.M1 * c[2]
    assert got == ((p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff)


def test_threshold_scale_and_the_two_ways_to_index_agree():
    assert ddc.threshold(0.0) == 0 and ddc.threshold(0.5) == 2**31 and ddc.threshold(0.1) == 429496729
    assert ddc.threshold(math.nextafter(1.0, 0.0)) == 2**32 - 1
    assert ddc.scale(0.5) == np.float32(2.0) and ddc.scale(0.1) == np.float32(1.0 / 0.9)
    first, count = ddc.KEEP_FIRST, ddc.KEEP_COUNT
    assert first >> 34 == 1 and count % 4 and count % 64  # the high counter word; no multiple of 4 or 64
    a = ddc.keep_range(ddc.SEED_KEEP, 1, first, count, 0.5)
    b = ddc.keep_elements(ddc.SEED_KEEP, 1, first + np.arange(count, dtype=np.uint64), 0.5)
    assert a.shape == (count,) and np.array_equal(a, b)
    # the counter's high word and the key's high word both matter
    assert not np.array_equal(a, ddc.keep_range(ddc.SEED_KEEP, 1, first - 2**34, count, 0.5))
    assert not np.array_equal(a, ddc.keep_range(ddc.SEED_KEEP & (2**63 - 1), 1, first, count, 0.5))
    assert ddc.keep_range(5, 0, 0, 1000, 0.0).all()


def test_seed_1234_keeps_4735_of_the_5285_sampled_elements():
    """every seventh element of the 17 x 17 x 128 tensor of stream 0 at p = 0.1"""
    total = 17 * 17 * 128
    sample = np.arange(0, total, 7, dtype=np.uint64)
    assert sample.size == 5285
    kept = int(ddc.keep_elements(1234, 0, sample, 0.1).sum())
    assert kept == 4735, kept
    assert kept == int(ddc.keep_range(1234, 0, 0, total, 0.1)[::7].sum())


@pytest.mark.parametrize("case", ddc.gpu_masks(), ids=lambda c: c[0])
def test_the_keep_rate_of_every_mask_the_gpu_tests_draw(case):
    label, seed, stream, first, count, p = case
    kept = int(ddc.keep_range(seed, stream, first, count, p).sum())
    bound = 5.0 * math.sqrt(count * p * (1.0 - p))
    print(f"{label}: kept {kept} of {count}, expected {count * (1.0 - p):.1f} +- {bound:.1f}")
    assert abs(kept - count * (1.0 - p)) <= bound


def test_the_masks_of_the_two_streams_and_of_two_seeds_differ():
    n = 4096
    base = ddc.keep_range(ddc.SEED_EDGE, 0, 0, n, 0.5)
    for other in (ddc.keep_range(ddc.SEED_EDGE, 1, 0, n, 0.5), ddc.keep_range(ddc.SEED_EDGE + 1, 0, 0, n, 0.5)):
        # independent fair bits agree on n / 2 places, standard deviation sqrt(n) / 2
        agree = int((base == other).sum())
        assert abs(agree - n / 2) <= 5.0 * math.sqrt(n) / 2.0, agree
    seeds = ddc.layer_seeds(torch.Generator().manual_seed(ddc.MODEL_GENERATOR_SEED), ddc.MODEL_LAYERS)
    assert len(set(seeds)) == ddc.MODEL_LAYERS and all(0 <= s < 2**63 - 1 for s in seeds)
    again = ddc.layer_seeds(torch.Generator().manual_seed(ddc.MODEL_GENERATOR_SEED), ddc.MODEL_LAYERS)
    assert seeds == again


def test_the_masks_have_the_layouts_of_the_two_logical_tensors():
    B, N, H, p = 2, 5, 3, 0.5
    m0 = ddc.edge_mask(9, p, B, N)
    b, i, j, unit = 1, 3, 4, 77
    e = ((b * N + i) * N + j) * 128 + unit
    assert bool(m0[b, i, j, unit] != 0) == bool(ddc.keep_elements(9, 0, [e], p)[0])
    m1 = ddc.attn_mask(9, p, B, H, N)
    b, d, h, q, k = 1, 1, 2, 4, 1
    e = (((b * 2 + d) * H + h) * N + q) * N + k
    assert bool(m1[b, d, h, q, k] != 0) == bool(ddc.keep_elements(9, 1, [e], p)[0])
    assert set(np.unique(m0.numpy())) == {np.float32(0.0), np.float32(2.0)}


def test_the_dropped_formulations_with_a_mask_of_ones_are_the_undropped_ones():
    import dual_backward_common as dbc
    args, _ = dbc.edge_case(2, 5, 2)
    ones = torch.ones((2, 5, 5, 128))
    assert torch.equal(ddc.edge_scores_torch(*args, ones), dg.edge_scores_torch(*args))
    att, _ = dbc.attention_case(2, 5, 2, 3, "scattered")
    got = ddc.attention_torch(*att, torch.ones((2, 2, 2, 5, 5)))
    want = dg.attention_torch(*att)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_the_switch_is_off_by_default_and_decides_the_rates_and_the_route():
    from gnn.dual_gnn import DualLayer
    model = dg.build_model("h32_H4_L2")
    layer = model.layers[0]
    assert DualLayer.fused_dropout is False and model.fused_dropout is False and model.dropout_generator is None
    assert layer._fused_dropout_rates() == (0.0, 0.0)
    model.fused_dropout = True
    assert all(m.fused_dropout for m in model.layers) and model.fused_dropout
    assert layer._fused_dropout_rates() == (0.0, 0.0)      # eval mode, and the fused training path is off
    model.train()
    assert layer._fused_dropout_rates() == (0.0, 0.0)      # the fused training path is off
    model.fused_attention_training = True
    assert layer._fused_dropout_rates() == (0.1, 0.1)
    layer.dropout.p = 0.0
    assert layer._fused_dropout_rates() == (0.1, 0.0)
    model.eval()
    assert layer._fused_dropout_rates() == (0.0, 0.0)      # eval mode never applies them
    g = torch.Generator().manual_seed(3)
    model.dropout_generator = g
    assert all(m.dropout_generator is g for m in model.layers) and model.dropout_generator is g
    edge, row, col, _ = dg.model_inputs("h32_H4_L2@pad")
    assert not layer.takes_fused_path(edge, row, col)      # CPU tensors, either way


def test_p_equal_to_one_takes_the_plain_path():
    """takes_fused_path looks at the device first, so the tensors here only claim to be on one"""
    model = dg.build_model("h32_H4_L2")
    model.fused_attention_training = True
    model.train()
    layer = model.layers[0]

    class OnDevice:
        is_cuda, requires_grad = True, False

    fake = OnDevice()
    assert layer.takes_fused_path(fake, fake, fake)
    layer.edge_mlp[2].p = 1.0
    assert layer.takes_fused_path(fake, fake, fake)         # the switch is off: routing as before
    layer.fused_dropout = True
    assert not layer.takes_fused_path(fake, fake, fake)
    layer.eval()
    assert layer.takes_fused_path(fake, fake, fake)
    layer.train()
    layer.edge_mlp[2].p, layer.dropout.p = 0.1, 1.0
    assert not layer.takes_fused_path(fake, fake, fake)


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_the_new_entries_are_declared_bound_and_exported(lib, name):
    assert re.search(r"\b%s\s*\(" % name, HEADER), name
    assert name in _hip.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5, float("nan"), float("inf")])
def test_a_bad_p_returns_minus_two_before_anything_else(lib, p):
    assert lib.lapwarm_dual_edge_scores_dropout(*([None] * 8), 2, 33, 4, 1, p, None) == -2
    assert lib.lapwarm_dual_attention_stats_dropout(*([None] * 14), 2, 33, 4, 8, 1, p, None) == -2
    assert lib.lapwarm_dual_attention_backward_dropout(*([None] * 24), 2, 33, 4, 8, None, 0, 1, p, None) == -2
    assert lib.lapwarm_dual_edge_scores_backward_dropout(*([None] * 13), 2, 33, 4, None, 0, 1, p, None) == -2
    assert lib.lapwarm_dual_dropout_keep(1, 0, 0, 16, p, None, None) == -2


def test_the_dropout_entries_return_the_argument_codes_of_the_entries_without(lib):
    P = 0x10000
    att = lambda b=2, n=33, h=4, s=P, ws=P, nbytes=1 << 30: lib.lapwarm_dual_attention_backward_dropout(  # noqa: E731
        s, *([P] * 5), None, None, *([P] * 16), b, n, h, 8, ws, nbytes, 1, 0.1, None)
    edge = lambda b=2, n=33, h=4, f=P, ws=P, nbytes=1 << 30: lib.lapwarm_dual_edge_scores_backward_dropout(  # noqa: E731
        f, *([P] * 6), None, *([P] * 5), b, n, h, ws, nbytes, 1, 0.1, None)
    for call in (att, edge):
        assert call(b=0) == -2 and call(n=0) == -2 and call(h=9) == -2 and call(ws=None) == -2
        assert call(n=16385) == -5
        assert call(nbytes=lib.lapwarm_dual_backward_workspace_bytes(2, 33, 4) - 1) == -1
    assert att(s=None) == -2 and edge(f=None) == -2
    fwd = lambda b=2, n=33, h=4, f=P: lib.lapwarm_dual_edge_scores_dropout(  # noqa: E731
        f, *([P] * 6), None, b, n, h, 1, 0.1, None)
    assert fwd(b=0) == -2 and fwd(h=9) == -2 and fwd(f=None) == -2 and fwd(n=16385) == -5
    stats = lambda n=33, s=P: lib.lapwarm_dual_attention_stats_dropout(  # noqa: E731
        s, *([P] * 5), None, None, *([P] * 6), 2, n, 4, 8, 1, 0.1, None)
    assert stats(n=0) == -2 and stats(s=None) == -2 and stats(n=16385) == -5
    assert lib.lapwarm_dual_dropout_keep(1, 0, 0, 16, 0.1, None, None) == -2
    assert lib.lapwarm_dual_dropout_keep(1, 0, 0, 0, 0.1, None, None) == 0       # nothing to write
    assert lib.lapwarm_dual_dropout_keep(1, 0, 0, 1 << 39, 0.1, P, None) == -2   # past the grid
