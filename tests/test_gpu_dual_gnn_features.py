"""The graph-feature kernels on the MI355X at the sizes where their loops repeat, against dual_gnn_common's
features_numpy (which test_dual_gnn_host.py shows bit-equal to the reference's recorded features).

gf_row_kernel runs 256 threads: every per-thread loop makes its second trip from n = 257, gf_sort's inner loop
repeats from npad = 1024 (n >= 513), and from n = 2049 (npad = 4096) the kernel needs 83 968 B of dynamic LDS, more
than the 64 KiB default.  Tolerances are those of test_gpu_dual_gnn.py's feature test (rtol 2e-6, atol 1e-9 per
channel); the two rank channels are compared exactly, as integers, tied inputs included: both sides rank the lower
index first among equal values.

n = 4096 is left out on purpose: features_numpy alone would take well over the few seconds a test here may take,
and n = 2049 already has the same npad, the same LDS size and the same launch path."""
import time

import numpy as np
import pytest
import torch

import dual_gnn_common as dg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 2e-6, 1e-9


def _device(C, u=None):
    from gnn.features import graph_features_device
    ud = None if u is None else torch.from_numpy(u).to(DEV)
    out = graph_features_device(torch.from_numpy(C).to(DEV), ud)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _signed(n, seed):
    """uniform in [-3, 3); row 0 begins with zeros of both signs, which rank by their index; u given"""
    rng = np.random.default_rng(seed)
    C = rng.random((n, n)) * 6.0 - 3.0
    C[0, :5] = [0.0, -0.0, 0.0, -0.0, 0.0]
    return C, rng.random(n) * 2.0 - 1.0


def _tied_integers(n, seed):
    rng = np.random.default_rng(seed)
    return np.floor(rng.random((n, n)) * 8.0) - 3.0, None


def _sparse_family(n, seed):
    """ordinary costs with about 30 % of the entries at 1e6, as the solver's sparse family has them"""
    rng = np.random.default_rng(seed)
    C = rng.random((n, n)) * 10.0
    C[rng.random((n, n)) < 0.3] = 1e6
    return C, None


def _uniform(n, seed):
    return np.random.default_rng(seed).random((n, n)) * 10.0, None


def _worst(got, want):
    """the largest |got - want| / (ATOL + RTOL |want|) over an array: at most 1 where allclose holds"""
    g, w = got.astype(np.float64), want.astype(np.float64)
    return float((np.abs(g - w) / (ATOL + RTOL * np.abs(w))).max())


def _compare(name, got, want, n):
    """device (edge, row, col) against features_numpy's: every channel within the tolerance, ranks exactly"""
    for w in want:
        assert np.isfinite(w).all(), name  # the reference itself is finite on every case
    edge, row, col = got
    assert edge.shape == (n, n, 10) and row.shape == (n, 14) and col.shape == (n, 14)
    assert edge.dtype == np.float32 and row.dtype == np.float32 and col.dtype == np.float32
    differ = sum(int((g != w).sum()) for g, w in zip(got, want))
    print(f"{name}: largest deviation in units of the tolerance: edge {_worst(edge, want[0]):.3e}, "
          f"row {_worst(row, want[1]):.3e}, col {_worst(col, want[2]):.3e} (bound 1); "
          f"{differ} of {sum(w.size for w in want)} float32 values differ from features_numpy's")
    for ch in range(10):
        assert np.allclose(edge[..., ch], want[0][..., ch], rtol=RTOL, atol=ATOL), (name, ch)
    for ch in range(14):
        assert np.allclose(row[:, ch], want[1][:, ch], rtol=RTOL, atol=ATOL), (name, "row", ch)
        assert np.allclose(col[:, ch], want[2][:, ch], rtol=RTOL, atol=ATOL), (name, "col", ch)
    for ch in (1, 2):
        assert np.array_equal(dg.integer_ranks(edge[..., ch], n), dg.integer_ranks(want[0][..., ch], n)), (name, ch)


CASES = {"signed_n255": (_signed, 255), "signed_n256": (_signed, 256), "signed_n257": (_signed, 257),
         "ties_int_n513": (_tied_integers, 513), "sparse_n300": (_sparse_family, 300)}


@pytest.mark.parametrize("name", list(CASES))
def test_graph_features_where_the_per_thread_loops_repeat(name):
    make, n = CASES[name]
    C, u = make(n, seed=n)
    want = dg.features_numpy(C, u)
    got = _device(C, u)
    _compare(name, got, want, n)
    if u is not None:
        assert got[0][..., 9].any()
        zeros = dg.integer_ranks(got[0][0, :5, 1], n)  # +0.0 and -0.0 are equal: the lower index first
        assert np.array_equal(np.diff(zeros), np.ones(4, dtype=np.int64))
    if name.startswith("ties"):
        k = dg.integer_ranks(got[0][..., 1], n)
        dg.assert_valid_stable_ranks(C[:8], k[:8])


def test_graph_features_of_a_batch_index_u_by_instance():
    B, n = 3, 33
    rng = np.random.default_rng(33)
    C = rng.random((B, n, n)) * 6.0 - 3.0
    u = rng.random((B, n)) * 2.0 - 1.0
    assert not np.array_equal(u[0], u[1]) and not np.array_equal(u[1], u[2])
    batched = _device(C, u)
    for b in range(B):
        one = _device(C[b], u[b])
        for got, alone in zip(batched, one):
            assert np.array_equal(got[b], alone), b
    _compare("B=3 n=33, instance 1", tuple(t[1] for t in batched), dg.features_numpy(C[1], u[1]), n)


def test_graph_features_with_lds_above_64k_and_later_calls_unchanged():
    """n = 2049: npad = 4096, 83 968 B of dynamic LDS through the limit that launch_graph_features raises once per
    process.  A small case run before and after it must give the same bits."""
    small_C, small_u = _signed(257, seed=257)
    before = _device(small_C, small_u)
    n = 2049
    C, _ = _uniform(n, seed=n)
    t0 = time.perf_counter()
    want = dg.features_numpy(C)
    t1 = time.perf_counter()
    got = _device(C)
    t2 = time.perf_counter()
    print(f"n = 2049: features_numpy {t1 - t0:.2f} s, device call and copy back {t2 - t1:.2f} s")
    _compare("uniform_n2049", got, want, n)
    assert not got[0][..., 9].any()
    after = _device(small_C, small_u)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
