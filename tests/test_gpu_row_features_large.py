"""The row-feature kernels (csrc/dense_sweeps.hip: row_features_kernel, row_features_ragged_kernel) on the MI355X
from n = 1025 to the cap of 16384, against the NumPy reference (oracle/features_np.py).

The matrices are tiled from the rows of tests/row_features_common.py, one per path of the kernel (what each row
reaches is asserted on the CPU by tests/test_row_features_host.py): 14 rows are uploaded and repeated on the
device, the reference is computed on the 14 rows, and every row of the device result is compared with the
expectation of the row it repeats.  Columns 0, 1, 4, 6, 11, 12 and the top-16 are equal to the float32 cast of the
reference; the other statistics are within test_row_features_batched's rtol = 3e-6, atol = 1e-9.

Sizes: 1025, 2048 (the benchmark's), 2049, 4096, 4097, the two on either side of 64 KiB of dynamic LDS
(4528 + 9 npad bytes, npad = n rounded up to even: 6778 and 6779), 16383 and 16384."""
import ctypes as ct
import functools

import numpy as np
import pytest

import row_features_common as rfc
from dense_sweeps_common import same
from oracle import features_np

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.0)


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    batch_on_device.cache_clear()
    uniform_results.cache_clear()


def tiled_on_device(rows, n, shift):
    """rows[tile_index(n, R, shift)] built on the device from one upload of the R rows."""
    import torch
    R = rows.shape[0]
    up = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    cyc = up[:R - 1].roll(-shift, 0)
    full, rem = divmod(n - 1, R - 1)
    C = torch.empty((n, n), dtype=torch.float64, device=up.device)
    C[:full * (R - 1)].view(full, R - 1, n).copy_(cyc.unsqueeze(0).expand(full, R - 1, n))
    C[full * (R - 1):n - 1].copy_(cyc[:rem])
    C[n - 1].copy_(up[R - 1])
    return C


@functools.lru_cache(maxsize=None)
def batch_on_device(n):
    """(B, n, n) fp64: instance b is tiled from instance_rows(base_rows(n), b).  Read-only by agreement."""
    import torch
    base = rfc.base_rows(n)
    mats = [tiled_on_device(rfc.instance_rows(base, b), n, rfc.INSTANCE_SHIFT[b]) for b in range(rfc.batch_of(n))]
    return mats[0].unsqueeze(0) if len(mats) == 1 else torch.stack(mats)


@functools.lru_cache(maxsize=None)
def uniform_results(n):
    """row_features_device on batch_on_device(n): (feat, topk) on the host, computed once and never modified."""
    import torch

    from gnn.features import row_features_device
    feat, topk = row_features_device(batch_on_device(n))
    torch.cuda.synchronize()
    feat, topk = feat.cpu().numpy(), topk.cpu().numpy()
    feat.setflags(write=False)
    topk.setflags(write=False)
    return feat, topk


@functools.lru_cache(maxsize=None)
def small_instance(n):
    """An n x n instance (n <= 3) of uniform costs, its device copy and its uniform-kernel result, checked
    against the reference here."""
    import torch

    from gnn.features import row_features_device
    C = np.random.default_rng([30, n]).random((n, n))
    Cd = torch.from_numpy(C).cuda()
    feat, topk = (t.cpu().numpy() for t in row_features_device(Cd))
    np.testing.assert_allclose(feat, features_np.compute_row_features(C), rtol=rfc.RTOL, atol=rfc.ATOL)
    assert np.array_equal(topk[:, :n], features_np.topk_smallest(C).astype(np.float32))
    assert np.isposinf(topk[:, n:]).all()
    return Cd, feat, topk


def instance0(n):
    """Instance 0 at size n: the device matrix and the uniform kernel's (feat, topk) for it."""
    if n <= 3:
        return small_instance(n)
    feat, topk = uniform_results(n)
    return batch_on_device(n)[0], feat[0], topk[0]


def check_against_reference(feat, topk, want, idx, names, tag):
    """feat (n, 21), topk (n, 16) of one instance whose row i repeats row idx[i] of the rows `want` was computed
    from.  Prints the largest relative error per column, then asserts."""
    n = feat.shape[0]
    exp = want.feat32[idx]
    errs = rfc.column_errors(feat[:, :13], exp)
    print(f"row features {tag}: max rel err per column " + " ".join(f"{c}:{e:.2e}" for c, e in enumerate(errs)))

    def rows_of(bad):
        return sorted({names[k] for k in idx[np.flatnonzero(bad)]})
    for col in rfc.EXACT_COLUMNS:
        bad = feat[:, col] != exp[:, col]
        assert not bad.any(), (tag, "column", col, rows_of(bad), feat[bad, col][:4], exp[bad, col][:4])
    bad = (topk != want.topk32[idx]).any(axis=1)
    assert not bad.any(), (tag, "top-16", rows_of(bad))
    bad = ~np.isclose(feat[:, :13], exp, rtol=rfc.RTOL, atol=rfc.ATOL)
    assert not bad.any(), (tag, "columns", np.flatnonzero(bad.any(axis=0)), rows_of(bad.any(axis=1)))
    np.testing.assert_allclose(feat[:, :13], exp, rtol=rfc.RTOL, atol=rfc.ATOL, err_msg=str(tag))
    assert np.array_equal(feat[:, 13:], features_np.positional_encodings(n)), tag


# ------------------------------------------------------------------------------------- against NumPy
@pytest.mark.parametrize("n", rfc.SIZES)
def test_every_row_against_numpy(n):
    R = len(rfc.RECIPES)
    if n == 1025:  # the device tiling is the host's
        for b in range(rfc.batch_of(n)):
            rows = rfc.instance_rows(rfc.base_rows(n), b)
            assert np.array_equal(batch_on_device(n)[b].cpu().numpy(),
                                  rows[rfc.tile_index(n, R, rfc.INSTANCE_SHIFT[b])])
    feat, topk = uniform_results(n)
    assert feat.shape == (rfc.batch_of(n), n, 21) and topk.shape == (rfc.batch_of(n), n, 16)
    for b in range(rfc.batch_of(n)):
        check_against_reference(feat[b], topk[b], rfc.expected(n, b), rfc.tile_index(n, R, rfc.INSTANCE_SHIFT[b]),
                                rfc.NAMES, f"n={n} b={b} lds={rfc.lds_bytes(n)}")


@pytest.mark.parametrize("n", (257, 4096))
def test_entropy_on_both_sides_of_its_threshold(n):
    """Column 5 of the two edge rows of n, and of the below-threshold row of n = 4096, which is closed-form at
    n = 257 and element-wise at n = 4096 (tests/test_row_features_host.py)."""
    import torch

    from gnn.features import row_features_device
    rows = rfc.entropy_rows(n)
    feat, topk = row_features_device(tiled_on_device(rows, n, 0))
    torch.cuda.synchronize()
    feat, topk = feat.cpu().numpy(), topk.cpu().numpy()
    want, idx = rfc.expected_rows(rows), rfc.tile_index(n, 3)
    print(f"entropy n={n}: kernel {feat[[0, 1, n - 1], 5]} reference {want.stats[:, 5]}")
    np.testing.assert_allclose(feat[:, 5], want.feat32[idx, 5], rtol=rfc.RTOL, atol=rfc.ATOL)
    check_against_reference(feat, topk, want, idx, ("above", "below", "below_of_4096"), f"entropy rows n={n}")


# --------------------------------------------------------------------------------------- ragged entry
def ragged_outputs_hold(o, sizes, N):
    """Every prefix of a raw ragged call's outputs is the uniform kernel's result for that instance, bit for bit,
    cost32 included, and every word outside the prefixes is its padding value."""
    import torch
    torch.cuda.synchronize()
    feat, topk = o["feat"].cpu().numpy(), o["topk"].cpu().numpy()
    assert (o["ret"].cpu().numpy() == 0).all()
    mask = o["mask"].cpu().numpy()
    for b, n in enumerate(sizes):
        Cd, f1, t1 = instance0(n)
        assert same(feat[b, :n], f1), (b, n, np.argwhere(feat[b, :n] != f1)[:4])
        assert same(topk[b, :n], t1), (b, n)
        assert (feat[b, n:] == 0).all() and np.isposinf(topk[b, n:]).all()
        assert mask[b].tolist() == [1] * n + [0] * (N - n)
        want = torch.zeros((N, N), dtype=torch.float32, device=Cd.device)
        want[:n, :n] = Cd.to(torch.float32)
        assert torch.equal(o["cost32"][b], want), (b, n)
        del want


@pytest.mark.parametrize("layout", ("packed", "padded"))
def test_ragged_prefixes_are_the_uniform_results(layout):
    import torch

    from gnn.features import ragged_pack
    from test_gpu_ragged_batch import raw_call
    sizes = [4097, 2048, 1, 1025]
    N = max(sizes)
    mats = [instance0(n)[0] for n in sizes]
    if layout == "packed":
        p = ragged_pack(mats)
        assert p.ld == 0
    else:  # NaN right of and below every prefix: nothing of it may be read
        Cp = torch.full((len(sizes), N, N), np.nan, dtype=torch.float64, device=mats[0].device)
        for b, (n, m) in enumerate(zip(sizes, mats)):
            Cp[b, :n, :n] = m
        p = ragged_pack(Cp, sizes=sizes)
        assert p.ld == N
    ragged_outputs_hold(raw_call(p), sizes, N)


def test_ragged_at_the_cap():
    from gnn.features import ragged_pack
    from test_gpu_ragged_batch import raw_call
    sizes = [16384, 3]
    ragged_outputs_hold(raw_call(ragged_pack([instance0(n)[0] for n in sizes])), sizes, 16384)


# ------------------------------------------------------------------------------- through the C ABI
def raw_uniform(C, stream=None, extra_rows=0):
    """lapwarm_row_features_batched on C (B, n, n) into outputs of B n + extra_rows rows filled with SENTINEL,
    with a workspace of 0xFF bytes.  Returns rc and the device outputs as (rows, 21) and (rows, 16)."""
    import torch

    from gnn.features import _posenc_device
    from lap import _hip
    lib = _hip.require_device()
    B, n, _ = C.shape
    rows = B * n + extra_rows
    feat = torch.full((rows, 21), float(SENTINEL), dtype=torch.float32, device=C.device)
    topk = torch.full((rows, 16), float(SENTINEL), dtype=torch.float32, device=C.device)
    nbytes = int(lib.lapwarm_sweep_workspace_bytes(B, n))
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=C.device)
    pos = _posenc_device(n, C.device)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(C.device) if stream is None else stream
    rc = lib.lapwarm_row_features_batched(C.data_ptr(), B, n, pos.data_ptr(), feat.data_ptr(), topk.data_ptr(),
                                          ws.data_ptr(), nbytes, ct.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    return rc, feat, topk


def test_lds_size_goes_up_down_and_up_again():
    """One process: n = 16384, n = 3, n = 16384 on a second stream; then the ragged entry at N = 2 and at
    N = 16384.  Every call returns 0 and every result at 16384 has the bits of the first."""
    import torch

    from gnn.features import ragged_pack
    from test_gpu_ragged_batch import raw_call
    C = batch_on_device(16384)
    f0, t0 = uniform_results(16384)
    small, fs, ts = small_instance(3)
    rc, feat, topk = raw_uniform(C)
    assert rc == 0 and same(feat.cpu().numpy(), f0[0]) and same(topk.cpu().numpy(), t0[0])
    rc, feat, topk = raw_uniform(small.unsqueeze(0))
    assert rc == 0 and same(feat.cpu().numpy(), fs) and same(topk.cpu().numpy(), ts)
    rc, feat, topk = raw_uniform(C, stream=torch.cuda.Stream(C.device))
    assert rc == 0 and same(feat.cpu().numpy(), f0[0]) and same(topk.cpu().numpy(), t0[0])
    ragged_outputs_hold(raw_call(ragged_pack([small_instance(2)[0], small_instance(1)[0]])), [2, 1], 2)
    ragged_outputs_hold(raw_call(ragged_pack([C[0], small])), [16384, 3], 16384)


@pytest.mark.parametrize("n", (2049, 16383))
def test_nothing_is_written_past_the_last_row(n):
    C, f1, t1 = instance0(n)
    rc, feat, topk = raw_uniform(C.unsqueeze(0), extra_rows=1)
    feat, topk = feat.cpu().numpy(), topk.cpu().numpy()
    assert rc == 0
    assert (feat[n:] == SENTINEL).all() and (topk[n:] == SENTINEL).all()
    assert same(feat[:n], f1) and same(topk[:n], t1)


@pytest.mark.parametrize("value,near_best", ((0.75, 1.0), (-0.75, 0.0)))
def test_counter_fields_of_a_constant_matrix_at_the_cap(value, near_best):
    """16384 near-best and 16384 column-best elements in every row: both fields of the packed counter are full.
    A positive constant is <= 1.1 x itself everywhere, a negative one nowhere."""
    import torch

    from gnn.features import row_features_device
    n = 16384
    feat, topk = row_features_device(torch.full((1, n, n), value, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    feat, topk = feat[0].cpu().numpy(), topk[0].cpu().numpy()
    assert (feat[:, 11] == np.float32(near_best)).all() and (feat[:, 12] == np.float32(1.0)).all()
    want = rfc.expected_rows(np.full((1, n), value))
    check_against_reference(feat, topk, want, np.zeros(n, dtype=np.int64), ("constant",), f"constant {value} n={n}")
