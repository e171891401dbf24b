"""The dense sweep kernels (column / row minima, project round, reduce costs, batched row features) and
the refinement aggregation on the MI355X, through the C ABI with torch CUDA tensors, against the NumPy
references of tests/dense_sweeps_common.py: above one trip of the 256-thread loops, at odd sizes, on the
scalar and the 16-byte column paths, with one-row last chunks, with instances that all differ.

Every workspace and every output buffer is filled with 0xFF bytes (NaN as fp64 and as float32) before a
call, so a word that is read or returned without having been written shows.  fp64 results are compared
exactly: each min or subtract is one fp64 operation, and the library is built without FMA contraction."""
import ctypes as ct

import numpy as np
import pytest

import dense_sweeps_common as dsc
from oracle import features_np

pytestmark = pytest.mark.gpu

SHAPE_IDS = [f"B{b}_n{n}" for b, n in dsc.SHAPES]


class Device:
    def __init__(self):
        import torch

        from lap import _hip
        assert torch.cuda.is_available(), "GPU tests need the MI355X"
        self.torch = torch
        self.lib = _hip.require_device()
        self.dev = torch.device("cuda:0")

    @property
    def stream(self):
        return ct.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def poisoned(self, shape, dtype):
        """A device buffer of 0xFF bytes."""
        t = self.torch.empty(shape, dtype=dtype, device=self.dev)
        t.view(self.torch.uint8).fill_(0xFF)
        return t

    def workspace(self, B, n):
        nbytes = self.lib.lapwarm_sweep_workspace_bytes(B, n)
        assert nbytes > 0
        return self.poisoned((nbytes,), self.torch.uint8), nbytes

    def put_off_by_8(self, a):
        """The same numbers 8 bytes into a larger allocation: data_ptr() % 16 == 8."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        buf = self.torch.empty((a.size + 3,), dtype=self.torch.float64, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        view = buf[1:1 + a.size].view(a.shape)
        view.copy_(self.torch.from_numpy(a))
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        return view

    def sync(self):
        self.torch.cuda.synchronize()

    # -- the four sweep operations, device tensors in, NumPy out
    def colmin(self, C, u):
        B, n, _ = C.shape
        ws, nbytes = self.workspace(B, n)
        out = self.poisoned((B, n), self.torch.float64)
        rc = self.lib.lapwarm_colmin_batched(C.data_ptr(), B, n, None if u is None else u.data_ptr(),
                                             out.data_ptr(), ws.data_ptr(), nbytes, self.stream)
        self.sync()
        assert rc == 0
        return out.cpu().numpy()

    def rowmin(self, C, v):
        B, n, _ = C.shape
        out = self.poisoned((B, n), self.torch.float64)
        rc = self.lib.lapwarm_rowmin_batched(C.data_ptr(), B, n, None if v is None else v.data_ptr(),
                                             out.data_ptr(), self.stream)
        self.sync()
        assert rc == 0
        return out.cpu().numpy()

    def project_round(self, C, u, v):
        """u, v updated in place on the device; returns (u, v, gmin) as NumPy."""
        B, n, _ = C.shape
        ws, nbytes = self.workspace(B, n)
        gmin = self.poisoned((B,), self.torch.float64)
        rc = self.lib.lapwarm_project_round_batched(C.data_ptr(), B, n, u.data_ptr(), v.data_ptr(),
                                                    gmin.data_ptr(), ws.data_ptr(), nbytes, self.stream)
        self.sync()
        assert rc == 0
        return u.cpu().numpy(), v.cpu().numpy(), gmin.cpu().numpy()

    def reduce_costs(self, C, u, v, shift_nonneg):
        B, n, _ = C.shape
        ws, nbytes = self.workspace(B, n)
        out = self.poisoned((B, n, n), self.torch.float64)
        gmin = self.poisoned((B,), self.torch.float64)
        rc = self.lib.lapwarm_reduce_costs_batched(C.data_ptr(), B, n, u.data_ptr(), v.data_ptr(),
                                                   int(shift_nonneg), out.data_ptr(), gmin.data_ptr(),
                                                   ws.data_ptr(), nbytes, self.stream)
        self.sync()
        assert rc == 0
        return out.cpu().numpy(), gmin.cpu().numpy()


@pytest.fixture(scope="module")
def gpu():
    return Device()


def mismatch(got, want):
    """Where two arrays differ, for the assertion message."""
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    idx = np.argwhere(bad)[:4]
    return [(tuple(int(t) for t in i), got[tuple(i)], want[tuple(i)]) for i in idx]


# ------------------------------------------------------------------------------- column minima
@pytest.mark.parametrize("B,n", dsc.SHAPES, ids=SHAPE_IDS)
def test_colmin_and_min_trick(gpu, B, n):
    """u NULL, u fp64 (C ABI) and u float32 (gnn.features.min_trick_device), then the same with C 8 bytes
    off 16-byte alignment, which must take the scalar kernel at even n too."""
    from gnn.features import min_trick_device
    for family in dsc.FAMILIES:
        C = dsc.plant_col_minima(dsc.costs(family, B, n))[0]
        u = dsc.small_duals(B, n)
        u32 = u.astype(np.float32)
        want_plain, want_u, want_u32 = dsc.colmin(C), dsc.colmin(C, u), dsc.colmin(C, u32)
        ud = gpu.put(u)
        aligned = gpu.put(C)
        assert aligned.data_ptr() % 16 == 0
        for where, Cd in (("aligned", aligned), ("off by 8", gpu.put_off_by_8(C))):
            got = gpu.colmin(Cd, None)
            assert dsc.same(got, want_plain), (family, where, "u NULL", mismatch(got, want_plain))
            got = gpu.colmin(Cd, ud)
            assert dsc.same(got, want_u), (family, where, "u fp64", mismatch(got, want_u))
            got = min_trick_device(Cd, gpu.put(u32)).cpu().numpy()
            assert dsc.same(got, want_u32), (family, where, "u float32", mismatch(got, want_u32))


# ------------------------------------------------------------------------------- row minima
@pytest.mark.parametrize("B,n", dsc.SHAPES, ids=SHAPE_IDS)
def test_rowmin(gpu, B, n):
    for family in dsc.FAMILIES:
        C = dsc.plant_row_minima(dsc.costs(family, B, n))[0]
        v = dsc.small_duals(B, n)
        Cd = gpu.put(C)
        got = gpu.rowmin(Cd, None)
        assert dsc.same(got, dsc.rowmin(C)), (family, "v NULL", mismatch(got, dsc.rowmin(C)))
        got = gpu.rowmin(Cd, gpu.put(v))
        assert dsc.same(got, dsc.rowmin(C, v)), (family, "v given", mismatch(got, dsc.rowmin(C, v)))


# ------------------------------------------------------------------------------- project round
@pytest.mark.parametrize("B,n", dsc.SHAPES, ids=SHAPE_IDS)
def test_project_round_three_calls(gpu, B, n):
    """Three consecutive rounds on seeds like make_features'; u, v and gmin after every call.  The last
    instance of every batch is feasible from the start (u, v unchanged, gmin >= 0); a batch of one is run a
    second time as that instance.  No finite instance has gmin < 0 after a round (see
    test_dense_sweeps_reference.py); a negative gmin goes through the same kernels in test_reduce_costs."""
    for family in dsc.FAMILIES:
        C = dsc.planted(family, B, n)
        Cd = gpu.put(C)
        for feasible in ([(B - 1,)] if B > 1 else [(), (0,)]):
            u, v = dsc.project_seeds(C, feasible=feasible)
            ud, vd = gpu.put(u), gpu.put(v)
            for call in range(3):
                wu, wv, wg = dsc.project_round(C, u, v)
                gu, gv, gg = gpu.project_round(Cd, ud, vd)
                tag = (family, feasible, call)
                assert dsc.same(gu, wu), (tag, "u", mismatch(gu, wu))
                assert dsc.same(gv, wv), (tag, "v", mismatch(gv, wv))
                assert dsc.same(gg, wg), (tag, "gmin", mismatch(gg, wg))
                if family in dsc.FINITE_FAMILIES:
                    for b in feasible:
                        assert np.array_equal(gu[b], u[b]) and np.array_equal(gv[b], v[b]) and gg[b] >= 0, tag
                u, v = wu, wv


# ------------------------------------------------------------------------------- reduce costs
@pytest.mark.parametrize("B,n", dsc.SHAPES, ids=SHAPE_IDS)
def test_reduce_costs(gpu, B, n):
    """shift_nonneg 0 and 1; instances whose unshifted minimum is negative, exactly 0 and positive (only the
    first is shifted).  out and gmin against features_np.reduce_costs and the minimum of its matrix."""
    for family in dsc.FAMILIES:
        C = dsc.planted(family, B, n)
        Cd = gpu.put(C)
        for shift in range(1 if B >= 3 else 3):
            u, v, kinds = dsc.reduce_seeds(C, shift)
            ud, vd = gpu.put(u), gpu.put(v)
            for shift_nonneg in (0, 1):
                want, wg = dsc.reduce_costs(C, u, v, bool(shift_nonneg))
                got, gg = gpu.reduce_costs(Cd, ud, vd, shift_nonneg)
                tag = (family, kinds, shift_nonneg)
                assert dsc.same(gg, wg), (tag, "gmin", mismatch(gg, wg))
                assert dsc.same(got, want), (tag, "out", mismatch(got, want))


# ------------------------------------------------------------------------------- NaN
def test_nan_propagates_as_in_numpy(gpu):
    """np.min and np.minimum propagate NaN, and so do the four sweep operations: a NaN in C, and a NaN in
    u or v, in one instance of three, at a column only the second trip of a thread reaches."""
    B, n = 3, 257
    C = dsc.planted("uniform", B, n)
    Cn = C.copy()
    Cn[1, 5, 256] = np.nan
    Cn[1, 200, 3] = np.nan
    u, v = dsc.project_seeds(C)
    un, vn = u.copy(), v.copy()
    un[2, 256] = np.nan
    vn[2, 130] = np.nan
    Cd, Cnd = gpu.put(C), gpu.put(Cn)
    for tag, Ch, Cx, uh, vh in (("NaN in C", Cn, Cnd, u, v), ("NaN in u", C, Cd, un, v), ("NaN in v", C, Cd, u, vn)):
        got = gpu.colmin(Cx, gpu.put(uh))
        assert dsc.same(got, dsc.colmin(Ch, uh)), (tag, "colmin", mismatch(got, dsc.colmin(Ch, uh)))
        got = gpu.rowmin(Cx, gpu.put(vh))
        assert dsc.same(got, dsc.rowmin(Ch, vh)), (tag, "rowmin", mismatch(got, dsc.rowmin(Ch, vh)))
        want = dsc.project_round(Ch, uh, vh)
        got = gpu.project_round(Cx, gpu.put(uh), gpu.put(vh))
        for name, g, w in zip(("u", "v", "gmin"), got, want):
            assert dsc.same(g, w), (tag, "project round", name, mismatch(g, w))
        for shift_nonneg in (0, 1):
            want, wg = dsc.reduce_costs(Ch, uh, vh, bool(shift_nonneg))
            got, gg = gpu.reduce_costs(Cx, gpu.put(uh), gpu.put(vh), shift_nonneg)
            assert dsc.same(gg, wg), (tag, "reduce gmin", shift_nonneg, mismatch(gg, wg))
            assert dsc.same(got, want), (tag, "reduce out", shift_nonneg, mismatch(got, want))
    got = gpu.colmin(Cnd, None)
    assert dsc.same(got, dsc.colmin(Cn)), ("NaN in C", "colmin, u NULL", mismatch(got, dsc.colmin(Cn)))
    got = gpu.rowmin(Cnd, None)
    assert dsc.same(got, dsc.rowmin(Cn)), ("NaN in C", "rowmin, v NULL", mismatch(got, dsc.rowmin(Cn)))


# ------------------------------------------------------------------------------- host entries
@pytest.mark.parametrize("n", [257, 513, 1025])
def test_host_entries_above_one_stride(gpu, n):
    from solvers import check_dual_feasible, project_feasible, reduce_costs, seed_row_col_minima
    from solvers.seed_baselines import _row_min
    for family in ("uniform", "integer"):
        C = dsc.planted(family, 1, n)[0]
        u0, v0 = (a[0] for a in dsc.project_seeds(C[None]))
        pu, pv = project_feasible(C, u0, v0)
        wu, wv = features_np.project_feasible(C, u0, v0)
        assert np.array_equal(pu, wu) and np.array_equal(pv, wv), family
        for shift in (True, False):
            assert np.array_equal(reduce_costs(C, u0, v0, shift), features_np.reduce_costs(C, u0, v0, shift)), family
        assert check_dual_feasible(C, pu, pv, tol=1e-8) is True
        with pytest.raises(AssertionError) as mine:
            check_dual_feasible(C, u0, v0)
        with pytest.raises(AssertionError) as theirs:
            features_np.check_dual_feasible(C, u0, v0)
        assert str(mine.value) == str(theirs.value)
        su, sv = seed_row_col_minima(C)
        wu, wv = features_np.seed_row_col_minima(C)
        assert np.array_equal(su, wu) and np.array_equal(sv, wv), family
        Cr = dsc.plant_row_minima(dsc.costs(family, 1, n))[0][0]
        assert np.array_equal(_row_min(Cr), Cr.min(axis=1)), family
        assert np.array_equal(_row_min(Cr, v0), (Cr - v0[None, :]).min(axis=1)), family


# ------------------------------------------------------------------------------- row features, batched
@pytest.mark.parametrize("B,n", [(3, 257), (2, 514)])
def test_row_features_batched(gpu, B, n):
    """Per instance against features_np.  Column 12 (how many entries of the row are their column's minimum)
    is the one that goes wrong when the column minima come from another instance."""
    from gnn.features import row_features_device
    pos = features_np.positional_encodings(n)
    for family in ("uniform", "integer", "sparse"):
        C = dsc.planted(family, B, n)
        for where, Cd in (("aligned", gpu.put(C)), ("off by 8", gpu.put_off_by_8(C))):
            feat, topk = row_features_device(Cd)
            gpu.sync()
            feat, topk = feat.cpu().numpy(), topk.cpu().numpy()
            for b in range(B):
                tag = (family, where, b)
                want = features_np.row_statistics(C[b]).astype(np.float32)
                for col in (0, 1, 4, 6, 11, 12):
                    assert np.array_equal(feat[b][:, col], want[:, col]), (tag, col)
                assert np.array_equal(topk[b], features_np.topk_smallest(C[b]).astype(np.float32)), tag
                np.testing.assert_allclose(feat[b][:, :13], want, rtol=3e-6, atol=1e-9, err_msg=str(tag))
                assert np.array_equal(feat[b][:, 13:], pos), tag


# ------------------------------------------------------------------------------- refinement aggregation
SENTINEL = np.float32(-12345.0)
TAIL = 16  # one block of rows


def _refine_call(gpu, top, u_pre, w1, b1, with_wsum):
    torch = gpu.torch
    rows, H = top.shape[0], w1.shape[0]
    out = torch.full((rows + TAIL, H), float(SENTINEL), dtype=torch.float32, device=gpu.dev)
    wsum = torch.full((rows + TAIL,), float(SENTINEL), dtype=torch.float32, device=gpu.dev)
    td, ud, wd, bd = gpu.put(top), gpu.put(u_pre), gpu.put(w1), gpu.put(b1)
    if with_wsum:
        rc = gpu.lib.lapwarm_refine_aggregate_wsum(td.data_ptr(), ud.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                                   out.data_ptr(), wsum.data_ptr(), rows, H, gpu.stream)
    else:
        rc = gpu.lib.lapwarm_refine_aggregate_batched(td.data_ptr(), ud.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                                      out.data_ptr(), rows, H, 0, gpu.stream)
    gpu.sync()
    assert rc == 0
    out, wsum = out.cpu().numpy(), wsum.cpu().numpy()
    assert (out[rows:] == SENTINEL).all(), "out written past `rows`"
    assert (wsum[rows:] == SENTINEL).all(), "wsum written past `rows`"
    if not with_wsum:
        assert (wsum == SENTINEL).all()
    return out[:rows], wsum[:rows]


@pytest.mark.parametrize("H", [2, 3, 64, 192, 257])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33, 257])
def test_refine_aggregate(gpu, rows, H):
    """lapwarm_refine_aggregate_wsum and lapwarm_refine_aggregate_batched (no wsum) against the float64
    restatement, on full, +inf-padded, all-+inf, -inf / NaN, tied and widely spread rows.

    Exact: a row without a finite value gives out == 0 and wsum == 0; nothing past `rows` is written; both
    entry points give the same `out`.  wsum of any other row is within 4 float32 ulps of 1.  Tolerance: the
    max-abs error of the same formula in PyTorch-CPU float32 on the same inputs, times 4 (another summation
    order, other expf / erff, all float32), or 1e-6 if that is larger -- separately for the inputs of moderate
    size (u_pre, w1, b1 ~ N(0, 1)) and the large ones (u_pre = +-1e3, and w1, b1 x 50 for the GELU tails),
    each pooled over the calls of one (rows, H).

    Measured on an MI355X, maxima over the 30 (rows, H): moderate inputs, kernel 2.745e-06 and PyTorch-CPU
    float32 2.745e-06; large inputs, kernel 7.883e-04 and PyTorch-CPU float32 9.763e-04 (values of order 1e3
    to 1e4).  Largest ratio kernel / CPU above the 1e-6 floor: 2.07 (rows=257, H=2, large)."""
    shifts = range(len(dsc.REFINE_KINDS)) if rows < len(dsc.REFINE_KINDS) else (0, 3)
    calls = {"moderate": [], "large": []}
    for s in shifts:
        calls["moderate"].append((dsc.refine_inputs(rows, seed=H, shift=s), dsc.refine_weights(H, seed=s)))
    for s in shifts:
        off = 1e3 if s % 2 == 0 else -1e3
        calls["large"].append((dsc.refine_inputs(rows, seed=H + 1, shift=s, u_offset=off), dsc.refine_weights(H, seed=s)))
        calls["large"].append((dsc.refine_inputs(rows, seed=H + 2, shift=s), dsc.refine_weights(H, seed=s, scale=50.0)))
    seen = set()
    for group, lst in calls.items():
        err_gpu = err_cpu = 0.0
        for (top, u_pre, kinds), (w1, b1) in lst:
            seen |= set(kinds)
            ref, wref = dsc.refine_aggregate_ref(top, u_pre, w1, b1)
            cpu, _ = dsc.refine_aggregate_f32(top, u_pre, w1, b1)
            out, wsum = _refine_call(gpu, top, u_pre, w1, b1, True)
            out2, _ = _refine_call(gpu, top, u_pre, w1, b1, False)
            assert np.array_equal(out, out2), (group, "the two entry points differ")
            dead = wref == 0
            assert dead.sum() == sum(k == "masked" for k in kinds)
            assert (out[dead] == 0).all() and (wsum[dead] == 0).all(), group
            assert (np.abs(wsum[~dead].astype(np.float64) - 1.0) <= 4 * np.spacing(np.float32(1.0))).all(), group
            assert np.isfinite(out).all()
            err_gpu = max(err_gpu, float(np.abs(out.astype(np.float64) - ref).max()))
            err_cpu = max(err_cpu, float(np.abs(cpu.astype(np.float64) - ref).max()))
        print(f"refine rows={rows} H={H} {group}: kernel {err_gpu:.3e}, PyTorch-CPU float32 {err_cpu:.3e}")
        assert err_gpu <= max(4.0 * err_cpu, 1e-6), (group, err_gpu, err_cpu)
    assert rows < 8 or seen == set(dsc.REFINE_KINDS)


def test_onegnn_forward_with_padded_topk_and_masked_rows(gpu):
    """OneGNN.forward on the device with topk_values= (n = 12: four +inf per row) and a mask with False rows,
    against the CPU restatement at the project's 1e-5; masked rows of u are exactly 0."""
    torch = gpu.torch
    from gnn import OneGNN
    from gnn.features import row_features_device
    from oracle import one_gnn_ref
    B, n = 2, 12
    C32 = np.random.RandomState(12).uniform(0.0, 1.0, (B, n, n)).astype(np.float32)
    torch.manual_seed(5)
    model = OneGNN(21, hidden=64, layers=2).eval()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(gpu.dev)
    feat, topk = row_features_device(gpu.put(C32.astype(np.float64)))
    assert torch.isposinf(topk[..., n:]).all() and torch.isfinite(topk[..., :n]).all()
    mask = torch.ones((B, n), dtype=torch.bool)
    mask[0, 0] = mask[0, 7] = mask[1, n - 1] = False
    with torch.no_grad():
        u = model(feat, topk_values=topk, mask=mask.to(gpu.dev))["u"].cpu()
    want = one_gnn_ref.forward(sd, feat.cpu(), torch.from_numpy(C32), mask)
    assert float((u - want).abs().max()) <= 1e-5
    assert (u[~mask] == 0).all()
