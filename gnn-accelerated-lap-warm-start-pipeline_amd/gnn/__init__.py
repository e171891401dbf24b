"""`gnn` -- the OneGNN warm-start model and its row features on the MI355X.

Import surface of the reference's harness (scripts/gnn_benchmark.py:51):
    from gnn import DualGNN, OneGNN, compute_features, compute_row_features, compute_row_features_torch
OneGNN and the two row-feature functions are the hot path and run on the device.  `DualGNN` and
`compute_features` (the O(n^2)-edge model and its features, SURVEY.md section 2: out of scope) are
importable names that raise NotImplementedError when USED, so that the harness' import line
succeeds and its OneGNN branch runs; a DualGNN checkpoint is reported, not silently mishandled."""
from .collate import DeviceBatch, collate_device
from .features import (compute_row_features, compute_row_features_torch, positional_encodings, ragged_pack,
                       RaggedPack, ROW_FEATURE_DIM, row_min_ragged)
from .one_gnn import OneGNN, ResidualBlock
from .pipeline import GNNPredictor, WarmStartPipeline, load_checkpoint

_OUT_OF_SCOPE = ("{} is the O(n^2)-edge DualGNN path of the reference; it is outside the warm-start hot path "
                 "(row features -> OneGNN -> min-trick -> lapjv_seeded) that this MI355X package implements")


class DualGNN:  # noqa: D101 - import-compatible placeholder
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(_OUT_OF_SCOPE.format("gnn.DualGNN"))


def compute_features(*args, **kwargs):
    raise NotImplementedError(_OUT_OF_SCOPE.format("gnn.compute_features"))


__all__ = ["OneGNN", "ResidualBlock", "DualGNN", "compute_features", "compute_row_features",
           "compute_row_features_torch", "positional_encodings", "ROW_FEATURE_DIM", "GNNPredictor",
           "WarmStartPipeline", "load_checkpoint", "collate_device", "DeviceBatch", "ragged_pack", "RaggedPack",
           "row_min_ragged"]
