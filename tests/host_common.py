"""Fixtures and helpers that several test files share.  conftest.py holds what pytest hands out by itself; this
module is imported by name, and a fixture is visible in a test file under the name that file imports it by
(`from host_common import shared_pipe as pipe`).  Every fixture here has module scope: one value per test file."""
import numpy as np
import pytest


# --------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def lib():
    """liblapwarm_hip.so through ctypes; no device needed."""
    from lap import _hip
    return _hip.load()


@pytest.fixture(scope="module")
def lib_or_skip():
    """`lib`, but a library that is not built skips the test instead of failing it."""
    from lap import _hip
    try:
        return _hip.load()
    except ImportError:
        pytest.skip("liblapwarm_hip.so is not built")


@pytest.fixture(scope="module")
def device_lib():
    """`lib`, and an error where no HIP device is visible."""
    from lap import _hip
    return _hip.require_device()


# --------------------------------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def pipe(torch_cuda):
    """A pipeline of the test file's own around an untrained default OneGNN."""
    from gnn import OneGNN, WarmStartPipeline
    return WarmStartPipeline(OneGNN(21), "cuda:0")


@pytest.fixture(scope="module")
def small_model_pipe():
    """A pipeline of the test file's own around a seeded one-layer OneGNN of width 32 in eval mode."""
    import torch

    from gnn import OneGNN, WarmStartPipeline
    torch.manual_seed(0)
    return WarmStartPipeline(OneGNN(21, hidden=32, layers=1).eval(), torch.device("cuda:0"))


@pytest.fixture(scope="module")
def shared_pipe():
    """The process-wide pipeline that the NumPy-facing helpers of `solvers` and `lap` use themselves."""
    from gnn.pipeline import shared_pipeline
    return shared_pipeline()


# --------------------------------------------------------------------------------------- helpers
def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def padded(mats, width):
    """(B, width, width) with NaN outside every prefix: a kernel that read there would show it."""
    C = np.full((len(mats), width, width), np.nan)
    for b, m in enumerate(mats):
        C[b, :m.shape[0], :m.shape[0]] = m
    return C
