"""The backward of DualGNN's fused attention without a GPU: the closed forms that include/lapwarm_hip.h documents
against fp64 autograd of dual_gnn_common.attention_torch / edge_scores_torch, the routing switch left off, the
workspace query's refusals and the header's declarations."""
import re

import numpy as np
import pytest
import torch

import dual_backward_common as dbc
import dual_gnn_common as dg
from conftest import ROOT
from host_common import lib  # noqa: F401
from lap import _hip

HEADER = (ROOT / "include" / "lapwarm_hip.h").read_text()
NEW_SYMBOLS = ("lapwarm_dual_attention_backward", "lapwarm_dual_edge_scores_backward",
               "lapwarm_dual_backward_workspace_bytes", "lapwarm_dual_attention_stats",
               "lapwarm_dual_attention_stats_ragged", "lapwarm_dual_backward_chunk")


@pytest.mark.parametrize("mask_kind", ["none", "scattered", "one_empty"])
@pytest.mark.parametrize("N", [1, 5, 17])
def test_attention_closed_form_is_autograd_of_the_forward(N, mask_kind):
    args, grads = dbc.attention_case(2, N, 3, 4, mask_kind, seed=1)
    want = dbc.attention_autograd(args, grads)
    got = dbc.attention_backward_ref(args, grads)
    for name in dbc.ATT_NAMES:
        ref = want[name].numpy()
        err = dbc.max_err(got[name], ref)
        print(f"N={N} {mask_kind} {name}: {err:.3e}")
        assert err <= 1e-12 * max(1.0, float(np.abs(ref).max())), name
    if args[6] is not None:
        keep = args[6].numpy()
        pair = keep[:, None, None, :, None] & keep[:, None, None, None, :]
        assert not got["dS"][~np.broadcast_to(pair, got["dS"].shape)].any()
        assert not got["da_row"][~np.broadcast_to(keep[:, None, :], got["da_row"].shape)].any()
        assert not got["d_row_val"][~keep].any() and not got["d_col_val"][~keep].any()


@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("N", [1, 5, 17])
def test_edge_scores_closed_form_is_autograd_of_the_forward(N, heads):
    args, dS = dbc.edge_case(2, N, heads, seed=1)
    want = dbc.edge_scores_autograd(args, dS)
    got = dbc.edge_scores_backward_ref(args, dS)
    for name in dbc.EDGE_NAMES:
        ref = want[name].numpy()
        err = dbc.max_err(got[name], ref)
        print(f"N={N} heads={heads} {name}: {err:.3e}")
        assert err <= 1e-12 * max(1.0, float(np.abs(ref).max())), name


CHUNK = 30720  # the hand-worked values below are for this chunk; the GPU tests ask the library


def test_ragged_wave_tiles_and_chunk_crossings_against_hand_worked_values(lib):
    assert lib.lapwarm_dual_backward_chunk() == CHUNK  # otherwise work the values below out again
    sizes = (130, 97, 130, 130)
    # 130 * ceil(130 / 16) = 130 * 9, 97 * 7
    assert dbc.ragged_wave_tiles(sizes, 130) == [1170, 679, 1170, 1170]
    # 1920 - (1170 + 679) = 71 = 7 * 9 + 8: row 7, its ninth group, the columns 128 and 129
    # 3840 - (1170 + 679 + 1170) = 821
    assert dbc.chunk_crossings(sizes, 130, CHUNK) == [(1920, 2, 71), (3840, 3, 821)]
    assert dbc.ragged_tile_edges(sizes, 130, 1920) == [(2, 7, 128), (2, 7, 129)]
    assert dbc.ragged_tile_edges(sizes, 130, 1919) == [(2, 7, j) for j in range(112, 128)]
    # sizes outside 1..N have no tile and contain no crossing
    padded = (130, 0, 97, 130, 131, 130)
    assert dbc.ragged_wave_tiles(padded, 130) == [1170, 0, 679, 1170, 0, 1170]
    assert dbc.chunk_crossings(padded, 130, CHUNK) == [(1920, 3, 71), (3840, 5, 821)]
    assert dbc.ragged_tile_edges(padded, 130, 1170) == [(2, 0, j) for j in range(16)]
    with pytest.raises(ValueError):
        dbc.ragged_tile_edges(padded, 130, 4189)
    # the sizes of the padded model case: 679 + 1170 = 1849, 71 tiles into the third instance
    assert dbc.chunk_crossings((97, 130, 130), 130, CHUNK) == [(1920, 2, 71)]
    # a chunk that starts with an instance: offset 0; one that starts with the end of the tiles: no crossing
    assert dbc.chunk_crossings((16, 16), 16, 256) == [(16, 1, 0)]
    assert dbc.chunk_crossings((16,), 16, 256) == []
    # the sizes every case had before: one chunk
    assert dbc.prefix_sizes(2, 130).tolist() == [130, 97]
    assert sum(dbc.ragged_wave_tiles(dbc.prefix_sizes(2, 130), 130)) == 1849 < CHUNK // 16
    assert dbc.chunk_crossings(dbc.prefix_sizes(2, 130), 130, CHUNK) == []


def test_uniform_tiles_probe_gradient_and_prefix_mask():
    assert dbc.uniform_tile_edges(2, 3, 0) == [(0, i, j) for i in range(3) for j in range(3)] + \
        [(1, i, j) for i in range(3) for j in range(3)][:7]
    assert dbc.uniform_tile_edges(2, 3, 1) == [(1, 2, 1), (1, 2, 2)]
    assert dbc.uniform_tile_edges(1, 248, 1920) == [(0, 123, 216 + k) for k in range(16)]  # 30720 = 123 * 248 + 216
    mask = dbc.prefix_mask((3, 0, 4, 2), 3)
    assert mask.tolist() == [[True] * 3, [False] * 3, [False] * 3, [True, True, False]]
    assert torch.equal(dbc.prefix_mask(dbc.prefix_sizes(2, 130), 130)[1], torch.arange(130) < 97)
    dS = torch.arange(2 * 2 * 2 * 3 * 3, dtype=torch.float32).reshape(2, 2, 2, 3, 3) + 1.0
    probe = dbc.probe_gradient(dS, [(1, 2, 0)])
    assert torch.equal(probe[1, :, :, 2, 0], dS[1, :, :, 2, 0]) and probe.count_nonzero() == 4
    # an explicit size list gives attention_case the prefix mask of those sizes and the numbers of the default case
    a, _ = dbc.attention_case(4, 3, 1, 2, "prefix", sizes=(3, 0, 4, 2))
    b, _ = dbc.attention_case(4, 3, 1, 2, "prefix")
    assert torch.equal(a[6], mask) and torch.equal(a[0], b[0]) and torch.equal(a[8], b[8])


def test_the_switch_is_off_by_default_and_routing_is_unchanged_then():
    from gnn.dual_gnn import DualLayer
    model = dg.build_model("h32_H4_L2")
    edge, row, col, _ = dg.model_inputs("h32_H4_L2@pad")
    assert model.fused_attention_training is False and DualLayer.fused_attention_training is False
    assert all(layer.fused_attention_training is False for layer in model.layers)
    assert not model.layers[0].takes_fused_path(edge, row, col)  # CPU tensors, either way
    model.fused_attention_training = True
    assert all(layer.fused_attention_training for layer in model.layers) and model.fused_attention_training
    assert not model.layers[0].takes_fused_path(edge, row, col)  # still CPU tensors
    model.fused_attention_training = False
    assert not any(layer.fused_attention_training for layer in model.layers)


def test_the_backward_workspace_query_refuses_bad_arguments(lib):
    q = lib.lapwarm_dual_backward_workspace_bytes
    chunk = lib.lapwarm_dual_backward_chunk()
    assert chunk > 0 and chunk % 16 == 0
    for bad in ((0, 33, 4), (32768, 33, 4), (2, 0, 4), (2, 16385, 4), (2, 33, 0), (2, 33, 9), (-1, 33, 4)):
        assert q(*bad) == 0, bad
    assert q(1, 1, 1) > 0 and q(2, 33, 8) % 256 == 0
    assert q(1, 3, 4) <= q(1, 17, 4) <= q(2, 130, 4) <= q(1, 1024, 4)
    # the rows of one chunk stay within 64 MiB and the whole is a constant beyond one chunk of edges
    assert chunk * (4 * 128 + 32) * 4 <= 64 << 20
    assert q(1, 1024, 4) == q(1, 2048, 4) <= (64 << 20) + (16 << 20)


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_the_new_entries_are_declared_bound_and_exported(lib, name):
    assert re.search(r"\b%s\s*\(" % name, HEADER), name
    assert name in _hip.SIGNATURES and hasattr(lib, name)


def test_the_backward_entries_return_argument_codes_before_any_device_work(lib):
    P = 0x10000
    att = lambda b=2, n=33, h=4, s=P, ws=P, nbytes=1 << 30: lib.lapwarm_dual_attention_backward(  # noqa: E731
        s, *([P] * 5), None, None, *([P] * 16), b, n, h, 8, ws, nbytes, None)
    edge = lambda b=2, n=33, h=4, f=P, ws=P, nbytes=1 << 30: lib.lapwarm_dual_edge_scores_backward(  # noqa: E731
        f, *([P] * 6), None, *([P] * 5), b, n, h, ws, nbytes, None)
    for call in (att, edge):
        assert call(b=0) == -2 and call(n=0) == -2 and call(h=9) == -2 and call(ws=None) == -2
        assert call(n=16385) == -5
        assert call(nbytes=lib.lapwarm_dual_backward_workspace_bytes(2, 33, 4) - 1) == -1
        assert lib.lapwarm_last_error().decode().startswith("workspace too small")
    assert att(s=None) == -2 and edge(f=None) == -2
