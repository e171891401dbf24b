"""The ragged batch entries without a GPU: the ABI surface, the workspace query, and the argument errors of the
Python wrappers, which are raised on the host before anything touches a device (so they read the same with and
without one)."""
import re

import numpy as np
import pytest

from conftest import ROOT

RAGGED = ("lapwarm_ragged_workspace_bytes", "lapwarm_colmin_ragged", "lapwarm_row_features_ragged")


def test_header_declares_and_library_exports_the_ragged_entries():
    from lap import _hip
    lib = _hip.load()
    header = (ROOT / "include" / "lapwarm_hip.h").read_text()
    declared = set(re.findall(r"\b(lapwarm_\w+)\s*\(", header))
    for name in RAGGED:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _hip.SIGNATURES, name


def test_workspace_query_is_monotone_and_zero_for_no_columns():
    from lap import _hip
    q = _hip.load().lapwarm_ragged_workspace_bytes
    assert q(1, 0) == 0 and q(0, 64) == 0 and q(4, 0) == 0
    assert q(1, 16385) == 0 and q(65536, 8) == 0  # outside what a call accepts
    batches = (1, 2, 3, 4, 7, 32, 33, 1000, 65535)
    widths = (1, 2, 17, 512, 513, 2048, 16384)
    for N in widths:
        sizes = [q(B, N) for B in batches]
        assert sizes[0] >= 8 * N, (N, sizes[0])  # at least the column minima
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (N, sizes)
    for B in batches:
        sizes = [q(B, N) for N in widths]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (B, sizes)


def _wrappers():
    from gnn import collate_device
    from gnn.features import ragged_pack, row_features_ragged

    def collate(costs):
        return collate_device([{"cost": c, "u": np.zeros(c.shape[0]), "v": np.zeros(c.shape[0])} for c in costs])

    # (WarmStartPipeline.predict_ragged and solve_many validate through the same ragged_pack, first thing)
    return {"row_features_ragged": row_features_ragged, "ragged_pack": ragged_pack, "collate_device": collate}


BAD = {
    "non_square": lambda: [np.zeros((3, 3)), np.zeros((3, 4))],
    "vector": lambda: [np.zeros(4)],
    "empty_matrix": lambda: [np.zeros((2, 2)), np.zeros((0, 0))],
    "empty_list": lambda: [],
    # a zero-stride view: 16385 x 16385 without the 2 GiB
    "n_above_16384": lambda: [np.broadcast_to(np.float64(0.0), (16385, 16385))],
    "batch_above_65535": lambda: [np.zeros((1, 1))] * 65536,
}


@pytest.mark.parametrize("entry", ("row_features_ragged", "ragged_pack", "collate_device"))
@pytest.mark.parametrize("bad", list(BAD))
def test_wrappers_reject_bad_arguments_before_any_device_call(entry, bad, monkeypatch):
    """The ValueError comes before the library is even asked for a device: require_device is replaced by a trap."""
    from lap import _hip

    def trap():
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(_hip, "require_device", trap)
    with pytest.raises(ValueError):
        _wrappers()[entry](BAD[bad]())


def test_padded_form_rejects_bad_arguments_before_any_device_call(monkeypatch):
    from gnn.features import row_features_ragged
    from lap import _hip

    def trap():
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(_hip, "require_device", trap)
    C = np.zeros((2, 4, 4))
    for costs, sizes in ((C, [4]), (C, [4, 5]), (C, [0, 4]), (np.zeros((2, 4, 3)), [3, 3]), (np.zeros((0, 4, 4)), [])):
        with pytest.raises(ValueError):
            row_features_ragged(costs, sizes=sizes)


def test_good_arguments_reach_the_no_device_error_without_a_gpu():
    from gnn.features import row_features_ragged
    from lap import _hip
    if _hip.load().lapwarm_device_count() > 0:
        return  # with a GPU the call runs; tests/test_gpu_ragged_batch.py covers it
    with pytest.raises(RuntimeError, match="no HIP device"):
        row_features_ragged([np.zeros((2, 2)), np.ones((3, 3))])
