"""DualGNN on mixed-size batches without a GPU: the argument codes of the four ragged entries and their order (every
recorded call returns before its first HIP call), the workspace query, and `sizes` on the plain path of the model."""
import pytest
import torch

import dual_gnn_common as dg
from host_common import lib  # noqa: F401
from lap import _hip

DEV = 1 << 20  # a non-null "device pointer" that is never dereferenced


def test_ragged_feature_workspace_is_zero_out_of_range_and_at_least_the_uniform_one(lib):
    q, uniform = lib.lapwarm_graph_features_ragged_workspace_bytes, lib.lapwarm_graph_features_workspace_bytes
    assert q(0, 8) == 0 and q(1, 0) == 0 and q(-1, 8) == 0 and q(1, 4097) == 0 and q(32768, 8) == 0
    for B, N in ((1, 1), (1, 17), (3, 65), (2, 513), (32767, 1), (1, 4096)):
        assert q(B, N) >= uniform(B, N) > 0, (B, N)
    assert q(2, 65) >= 2 * 65 * 65 * (8 + 2 * 4)  # the transposed copy and the two rank planes, padded stride


def test_graph_features_ragged_argument_codes_come_in_the_house_order(lib):
    f = lib.lapwarm_graph_features_ragged
    need = lib.lapwarm_graph_features_ragged_workspace_bytes(2, 17)

    def call(C=DEV, offs=DEV, sizes=DEV, ld=0, B=2, N=17, u=None, pos=DEV, pos_off=DEV, edge=DEV, row=DEV, col=DEV,
             mask=DEV, ret=DEV, ws=DEV, nbytes=need):
        return f(C, offs, sizes, ld, B, N, u, pos, pos_off, edge, row, col, mask, ret, ws, nbytes, None)

    # dimensions first: -2 for batch or N out of range (also with a null pointer and a short workspace behind them)
    assert call(B=0) == -2 and call(B=32768) == -2 and call(N=0) == -2 and call(ld=-1) == -2
    assert call(B=0, C=None, nbytes=0) == -2
    # then N above the limit of the graph features
    assert call(N=4097) == -5 and call(N=4097, C=None, nbytes=0) == -5
    # then null pointers (u may be null), before the workspace size
    for name in ("C", "offs", "sizes", "pos", "pos_off", "edge", "row", "col", "mask", "ret", "ws"):
        assert call(**{name: None}) == -2, name
        assert call(**{name: None}, nbytes=0) == -2, name
    # then the workspace, with its text
    assert call(nbytes=need - 1) == -1
    assert _hip.last_error().startswith("workspace too small")
    assert f"{need - 1} < {need}" in _hip.last_error()


def test_ragged_attention_entries_argument_codes_come_in_the_house_order(lib):
    es = lib.lapwarm_dual_edge_scores_ragged

    def scores(sizes=DEV, out=DEV, B=1, n=8, heads=4, first=DEV):
        return es(first, DEV, DEV, DEV, DEV, DEV, out, sizes, B, n, heads, None)

    assert scores(B=0) == -2 and scores(B=32768) == -2 and scores(n=0) == -2
    assert scores(heads=0) == -2 and scores(heads=9) == -2
    assert scores(n=16385) == -5 and scores(n=16385, sizes=None) == -5
    assert scores(B=0, n=16385) == -2  # the range of batch and heads comes before the limit of n
    assert scores(sizes=None) == -2 and scores(out=None) == -2 and scores(first=None) == -2
    at = lib.lapwarm_dual_attention_ragged

    def attn(sizes=DEV, last=DEV, B=1, n=8, heads=4, D=8):
        return at(DEV, DEV, DEV, DEV, DEV, DEV, sizes, DEV, DEV, DEV, last, B, n, heads, D, None)

    assert attn(B=0) == -2 and attn(B=32768) == -2 and attn(n=0) == -2 and attn(heads=0) == -2
    assert attn(heads=65536) == -2 and attn(D=0) == -2
    assert attn(n=16385) == -5 and attn(n=16385, sizes=None) == -5
    assert attn(sizes=None) == -2 and attn(last=None) == -2


def _padded_case():
    model = dg.build_model("h32_H4_L2")
    edge, row, col, mask = dg.model_inputs("h32_H4_L2@pad")
    sizes = mask.sum(dim=1).to(torch.int32)
    n_pad = mask.shape[1]
    assert torch.equal(mask, torch.arange(n_pad)[None] < sizes[:, None])  # the fixture's mask is a prefix mask
    assert int(sizes.min()) < n_pad
    return model, edge, row, col, mask, sizes


def test_sizes_on_the_plain_path_equal_the_prefix_mask_exactly():
    model, edge, row, col, mask, sizes = _padded_case()
    assert not model.layers[0].takes_fused_path(edge, row, col)
    with torch.no_grad():
        want = model(edge, row, col, mask)
        from_sizes = model(edge, row, col, sizes=sizes)
        both = model(edge, row, col, mask, sizes=sizes)
        layer = model.layers[0]
        nodes = (model.row_encoder(row), model.col_encoder(col))
        plain = layer(edge, *nodes, mask)
        sized = layer(edge, *nodes, mask, sizes)
    for k in ("u", "v_hint"):
        assert torch.equal(from_sizes[k], want[k]) and torch.equal(both[k], want[k]), k
    assert torch.equal(plain[0], sized[0]) and torch.equal(plain[1], sized[1])


def test_a_mask_that_disagrees_with_the_sizes_and_bad_sizes_raise():
    model, edge, row, col, mask, sizes = _padded_case()
    wrong = mask.clone()
    wrong[0, 0] = not bool(wrong[0, 0])
    with torch.no_grad():
        with pytest.raises(ValueError, match="prefix mask"):
            model(edge, row, col, wrong, sizes=sizes)
        with pytest.raises(ValueError, match="prefix mask"):
            model(edge, row, col, mask[:, :-1], sizes=sizes)
        with pytest.raises(ValueError, match="prefix mask"):
            model(edge, row, col, mask, sizes=sizes - 1)
        with pytest.raises(TypeError, match="int32"):
            model(edge, row, col, sizes=sizes.to(torch.int64))
        with pytest.raises(ValueError, match="sizes must be"):
            model(edge, row, col, sizes=sizes[:-1])


def test_the_ragged_names_are_reachable_and_the_limit_is_checked_before_any_device_work():
    import numpy as np

    import gnn.features
    import gnn.pipeline
    assert callable(gnn.features.graph_features_packed) and callable(gnn.features.graph_features_ragged)
    assert gnn.features.RaggedGraphFeatures.__slots__ == ("edge", "row", "col", "mask", "sizes", "ret")
    assert callable(gnn.pipeline._predict_packed_dual)
    assert "not available" not in gnn.pipeline.DualWarmStartPipeline.__doc__
    big = np.lib.stride_tricks.as_strided(np.zeros(1), shape=(4097, 4097), strides=(0, 0))
    with pytest.raises(ValueError, match="4096"):
        gnn.features.graph_features_ragged([big, np.zeros((2, 2))])
