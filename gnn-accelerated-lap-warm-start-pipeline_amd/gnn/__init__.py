"""`gnn` -- the warm-start models and their features on the MI355X.

Import surface of the reference's harness (scripts/gnn_benchmark.py:51):
    from gnn import DualGNN, OneGNN, compute_features, compute_row_features, compute_row_features_torch
OneGNN and the two row-feature functions run on the device under these names.  `gnn.DualGNN` and
`gnn.compute_features` are still placeholders that raise NotImplementedError when USED (tests/test_host_logic.py
pins that), so that the harness' import line succeeds and its OneGNN branch runs; a DualGNN checkpoint handed to
`load_checkpoint` is reported, not silently mishandled.

The DualGNN path itself is implemented and runs on the device, under names that the pinned ones are not bound to
(the `lapmod_sparse` precedent): `gnn.dual_gnn.DualGNN`, `gnn.dual_gnn.DualLayer`, `gnn.features.compute_features`,
`gnn.features.graph_features_device`, `gnn.load_dual_checkpoint`, `gnn.pipeline.DualWarmStartPipeline` and
`gnn.pipeline.DualGNNPredictor`.  Once tests/test_host_logic.py stops pinning the three names, the routing is:
    1. here:  `from .dual_gnn import DualGNN` and `from .features import compute_features` replace the two
       placeholders below;
    2. `pipeline.load_checkpoint`: an `architecture` other than "one_gnn" returns `load_dual_checkpoint(path, device)`;
    3. `run_harness.py`: a DualGNN model gets `DualGNNPredictor`, a OneGNN model `GNNPredictor`."""
from .collate import DeviceBatch, collate_device
from .features import (compute_row_features, compute_row_features_torch, positional_encodings, ragged_pack,
                       RaggedPack, ROW_FEATURE_DIM, row_min_ragged)
from .one_gnn import OneGNN, ResidualBlock
from .pipeline import GNNPredictor, WarmStartPipeline, load_checkpoint, load_dual_checkpoint
from .synthetic import DEFAULT_PARAMS, FAMILY_IDS, SyntheticStream, synthetic_pack

_OUT_OF_SCOPE = ("{} is a placeholder that keeps the reference harness' import line working; the O(n^2)-edge DualGNN "
                 "path runs on the MI355X as {} (see the `gnn` docstring for the routing)")


class DualGNN:  # noqa: D101 - import-compatible placeholder
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(_OUT_OF_SCOPE.format("gnn.DualGNN", "gnn.dual_gnn.DualGNN"))


def compute_features(*args, **kwargs):
    raise NotImplementedError(_OUT_OF_SCOPE.format("gnn.compute_features", "gnn.features.compute_features"))


__all__ = ["OneGNN", "ResidualBlock", "DualGNN", "compute_features", "compute_row_features",
           "compute_row_features_torch", "positional_encodings", "ROW_FEATURE_DIM", "GNNPredictor",
           "WarmStartPipeline", "load_checkpoint", "collate_device", "DeviceBatch", "ragged_pack", "RaggedPack",
           "row_min_ragged", "FAMILY_IDS", "DEFAULT_PARAMS", "synthetic_pack", "SyntheticStream"]
