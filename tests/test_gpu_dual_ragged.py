"""DualGNN on mixed-size batches on the MI355X: the ragged graph features, the size-aware edge scores and attention
against the uniform entries bit for bit, the model with `sizes` against the model with the prefix mask, and
predict_ragged / solve_many of a DualWarmStartPipeline against the per-instance calls and the CPU solver oracle."""
import ctypes as ct

import numpy as np
import pytest
import torch

import dual_gnn_common as dg
from host_common import device_lib as lib  # noqa: F401
from host_common import padded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 2e-6, 1e-9  # test_gpu_dual_gnn_features.py's tolerance against features_numpy


def _stream():
    return ct.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _matrices(sizes, seed):
    """signed costs; the first row of every instance of five or more columns begins with zeros of both signs"""
    rng = np.random.default_rng(seed)
    mats = []
    for n in sizes:
        C = rng.random((n, n)) * 6.0 - 3.0
        if n >= 5:
            C[0, :5] = [0.0, -0.0, 0.0, -0.0, 0.0]
        mats.append(C)
    return mats


def _alone(C, u=None):
    """graph_features_device of one instance -> NumPy edge, row, col"""
    from gnn.features import graph_features_device
    ud = None if u is None else torch.from_numpy(np.ascontiguousarray(u)).to(DEV)
    out = graph_features_device(torch.from_numpy(C).to(DEV), ud)
    return tuple(t.cpu().numpy() for t in out)


def _check_ragged_features(f, sizes, alone):
    """every prefix equals the instance's own call bit for bit, everything else is exactly 0, the mask is the prefix"""
    N = max(sizes)
    edge, row, col = f.edge.cpu().numpy(), f.row.cpu().numpy(), f.col.cpu().numpy()
    mask = f.mask.cpu().numpy()
    assert edge.shape == (len(sizes), N, N, 10) and row.shape == col.shape == (len(sizes), N, 14)
    assert mask.dtype == np.bool_ and edge.dtype == row.dtype == col.dtype == np.float32
    for b, n in enumerate(sizes):
        e1, r1, c1 = alone[b]
        assert np.array_equal(edge[b, :n, :n], e1), b
        assert np.array_equal(row[b, :n], r1) and np.array_equal(col[b, :n], c1), b
        assert not edge[b, n:].any() and not edge[b, :, n:].any(), b
        assert not row[b, n:].any() and not col[b, n:].any(), b
        assert mask[b, :n].all() and not mask[b, n:].any(), b
        edge[b, :n, :n], row[b, :n], col[b, :n] = 0.0, 0.0, 0.0
    # no NaN and no -0.0 hides in the padding
    for t in (edge, row, col):
        assert not t.view(np.uint32).any()


# ---- 1. features ------------------------------------------------------------------------------------------------

FEATURE_SIZES = (513, 1, 2, 31, 32, 33, 255, 256, 257)


@pytest.fixture(scope="module")
def feature_case():
    """The cost matrices, their u, and what graph_features_device gives every instance alone, with u and without:
    computed once for the four layouts and argument sets below, and left unchanged."""
    mats = _matrices(FEATURE_SIZES, seed=513)
    rng = np.random.default_rng(7)
    us = [rng.random(n) * 2.0 - 1.0 for n in FEATURE_SIZES]
    alone = {True: [_alone(C, u) for C, u in zip(mats, us)], False: [_alone(C) for C in mats]}
    return mats, us, alone


@pytest.mark.parametrize("layout", ["packed", "padded"])
@pytest.mark.parametrize("with_u", [True, False], ids=["u", "no_u"])
def test_ragged_graph_features_equal_the_uniform_call_per_instance_bit_for_bit(feature_case, layout, with_u):
    from gnn.features import graph_features_ragged
    mats, us, alone = feature_case
    N = max(FEATURE_SIZES)
    u = None
    if with_u:
        uh = np.full((len(mats), N), np.nan)  # beyond a prefix u is not read
        for b, ub in enumerate(us):
            uh[b, :len(ub)] = ub
        u = torch.from_numpy(uh).to(DEV)
    if layout == "packed":
        f = graph_features_ragged(mats, u, device=DEV)
    else:
        f = graph_features_ragged(padded(mats, N), u, device=DEV, sizes=FEATURE_SIZES)
    torch.cuda.synchronize()
    assert f.ret.cpu().tolist() == [0] * len(mats)
    assert f.sizes.cpu().tolist() == list(FEATURE_SIZES)
    _check_ragged_features(f, FEATURE_SIZES, alone[with_u])
    assert bool(f.edge[..., 9].any()) == with_u
    # one instance against NumPy as well, at the tolerance of the uniform kernel's tests and with exact ranks
    b = FEATURE_SIZES.index(257)
    want = dg.features_numpy(mats[b], us[b] if with_u else None)
    got = (f.edge[b, :257, :257].cpu().numpy(), f.row[b, :257].cpu().numpy(), f.col[b, :257].cpu().numpy())
    for g, w in zip(got, want):
        assert np.allclose(g, w, rtol=RTOL, atol=ATOL)
    for ch in (1, 2):
        assert np.array_equal(dg.integer_ranks(got[0][..., ch], 257), dg.integer_ranks(want[0][..., ch], 257))


# ---- 2. an empty instance ------------------------------------------------------------------------------------------

def test_an_empty_instance_gets_ret_2_and_zeros_and_leaves_its_neighbours_alone():
    from gnn.features import RaggedPack, graph_features_packed, ragged_pack
    outer = _matrices((33, 17), seed=33)
    pack = ragged_pack([outer[0], np.ones((1, 1)), outer[1]], DEV)  # the middle instance holds one element ...
    sizes = torch.tensor([33, 0, 17], dtype=torch.int32, device=DEV)  # ... and is given the size 0
    empty = RaggedPack(pack.C, pack.offsets, sizes, pack.pos_off, pack.posenc, pack.ld, pack.N, [33, 0, 17])
    f = graph_features_packed(empty)
    torch.cuda.synchronize()
    assert f.ret.cpu().tolist() == [0, 2, 0]
    zeros = tuple(np.zeros(s, np.float32) for s in ((0, 0, 10), (0, 14), (0, 14)))
    _check_ragged_features(f, (33, 0, 17), [_alone(outer[0]), zeros, _alone(outer[1])])
    assert not f.mask[1].any()


# ---- 3. dynamic LDS above 64 KiB -----------------------------------------------------------------------------------

def test_ragged_graph_features_with_lds_above_64k():
    """N = 2049: the row kernel is launched with the 83 968 B of npad = 4096, and the instance of 257 lays its own
    npad = 512 out inside them."""
    from gnn.features import graph_features_ragged
    sizes = (2049, 257)
    rng = np.random.default_rng(2049)
    mats = [rng.random((n, n)) * 10.0 for n in sizes]
    f = graph_features_ragged(mats, device=DEV)
    torch.cuda.synchronize()
    assert f.ret.cpu().tolist() == [0, 0]
    _check_ragged_features(f, sizes, [_alone(C) for C in mats])


# ---- 4. edge scores -------------------------------------------------------------------------------------------------

def _nan_pattern(count):
    """quiet NaNs with the element's index in the payload: a changed element shows even if a NaN was written"""
    bits = torch.arange(count, dtype=torch.int32) % (1 << 22) + 0x7FC00000
    return bits.view(torch.float32)


@pytest.mark.parametrize("heads", [4, 8])
def test_ragged_edge_scores_equal_the_uniform_entry_on_the_prefixes_and_write_nothing_else(lib, heads):
    sizes, N = (150, 97, 1, 16, 17), 150
    B = len(sizes)
    g = torch.Generator().manual_seed(150 + heads)
    edge = torch.rand((B, N, N, 10), generator=g) * 2.0 - 0.5
    for b, n in enumerate(sizes):  # zero outside the prefixes, as the ragged features leave it
        edge[b, n:] = 0.0
        edge[b, :, n:] = 0.0
    W1 = (torch.rand((128, 10), generator=g) - 0.5) * 0.6
    b1 = (torch.rand((128,), generator=g) - 0.5) * 0.2
    W2 = (torch.rand((128, 128), generator=g) - 0.5) * 0.18
    b2 = (torch.rand((128,), generator=g) - 0.5) * 0.2
    G = (torch.rand((2 * heads, 128), generator=g) - 0.5) * 0.3
    d = [t.to(DEV).contiguous() for t in (edge, W1, b1, W2, b2, G)]
    count = B * 2 * heads * N * N
    pattern = _nan_pattern(count)
    uniform = pattern.to(DEV)
    rc = lib.lapwarm_dual_edge_scores(*(t.data_ptr() for t in d), uniform.data_ptr(), B, N, heads, _stream())
    assert rc == 0
    ragged = pattern.to(DEV)
    sizes_d = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    rc = lib.lapwarm_dual_edge_scores_ragged(*(t.data_ptr() for t in d), ragged.data_ptr(), sizes_d.data_ptr(), B, N,
                                             heads, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    uniform = uniform.cpu().reshape(B, 2 * heads, N, N)
    ragged = ragged.cpu().reshape(B, 2 * heads, N, N)
    untouched = pattern.reshape(B, 2 * heads, N, N).view(torch.int32)
    assert torch.isfinite(uniform).all()
    inside = torch.zeros((B, 1, N, N), dtype=torch.bool)
    for b, n in enumerate(sizes):
        inside[b, :, :n, :n] = True
        assert torch.equal(ragged[b, :, :n, :n], uniform[b, :, :n, :n]), b
    inside = inside.expand(B, 2 * heads, N, N)
    assert torch.equal(ragged.view(torch.int32)[~inside], untouched[~inside])


# ---- 5. attention ---------------------------------------------------------------------------------------------------

def _attention_inputs(sizes, N, H, D, seed):
    B = len(sizes)
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g) * 2.0 - 1.0  # noqa: E731
    t = dict(scores=r(B, 2, H, N, N) * 3.0, a_row=r(B, H, N), c_row=r(B, H, N), a_col=r(B, H, N), c_col=r(B, H, N),
             kbias=r(2 * H), row_val=r(B, N, H * D), col_val=r(B, N, H * D))
    return {k: v.to(DEV).contiguous() for k, v in t.items()}


def _attention(lib, symbol, t, selector, B, N, H, D):
    row_msg = torch.full((B, N, H * D), float("nan"), dtype=torch.float32, device=DEV)
    col_msg = torch.full((B, N, H * D), float("nan"), dtype=torch.float32, device=DEV)
    rc = getattr(lib, symbol)(t["scores"].data_ptr(), t["a_row"].data_ptr(), t["c_row"].data_ptr(),
                              t["a_col"].data_ptr(), t["c_col"].data_ptr(), t["kbias"].data_ptr(), selector.data_ptr(),
                              t["row_val"].data_ptr(), t["col_val"].data_ptr(), row_msg.data_ptr(), col_msg.data_ptr(),
                              B, N, H, D, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return row_msg.cpu(), col_msg.cpu()


@pytest.mark.parametrize("N,sizes,H,D", [(130, (130, 65, 64, 1), 2, 32), (17, (17, 5), 1, 136)])
def test_ragged_attention_equals_the_prefix_mask_bit_for_bit_and_never_reads_outside(lib, N, sizes, H, D):
    B = len(sizes)
    t = _attention_inputs(sizes, N, H, D, seed=N * 100 + H)
    mask = torch.zeros((B, N), dtype=torch.bool)
    outside = torch.ones((B, 1, 1, N, N), dtype=torch.bool)
    for b, n in enumerate(sizes):
        mask[b, :n] = True
        outside[b, :, :, :n, :n] = False
    want = _attention(lib, "lapwarm_dual_attention", t, mask.to(torch.uint8).to(DEV), B, N, H, D)
    poisoned = dict(t)
    poisoned["scores"] = t["scores"].masked_fill(outside.to(DEV), float("nan"))
    sizes_d = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    got = _attention(lib, "lapwarm_dual_attention_ragged", poisoned, sizes_d, B, N, H, D)
    again = _attention(lib, "lapwarm_dual_attention_ragged", poisoned, sizes_d, B, N, H, D)
    for g, a, w in zip(got, again, want):  # the row messages, then the column messages
        assert torch.isfinite(g).all()
        assert torch.equal(g, w) and torch.equal(g, a)
        assert not g[~mask].view(torch.int32).any()  # padded queries: exactly +0
        assert g[mask].any()


# ---- 6. the model ---------------------------------------------------------------------------------------------------

def test_fused_forward_with_sizes_equals_the_fused_forward_with_the_prefix_mask():
    """The masked case of test_gpu_dual_gnn.py (B = 3, N = 150, sizes (150, 97, 1), hidden 64, 2 layers, 8 heads)."""
    from gnn.dual_gnn import DualGNN
    sizes, N = (150, 97, 1), 150
    rng = np.random.default_rng(150)
    edge = np.zeros((len(sizes), N, N, 10), np.float32)
    row = np.zeros((len(sizes), N, 14), np.float32)
    col = np.zeros_like(row)
    mask = torch.zeros((len(sizes), N), dtype=torch.bool)
    for b, n in enumerate(sizes):
        edge[b, :n, :n], row[b, :n], col[b, :n] = dg.features_numpy(rng.random((n, n)) * 10.0)
        mask[b, :n] = True
    torch.manual_seed(12)
    model = DualGNN(hidden_dim=64, layers=2, heads=8).eval().to(DEV)
    e, r, c = (torch.from_numpy(t).to(DEV) for t in (edge, row, col))
    m = mask.to(DEV)
    s = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        assert model.layers[0].takes_fused_path(e, r, c)
        want = model(e, r, c, m)
        got = model(e, r, c, m, sizes=s)
        built = model(e, r, c, sizes=s)  # the mask is built from the sizes
        with pytest.raises(ValueError, match="prefix mask"):
            model(e, r, c, ~m, sizes=s)
    torch.cuda.synchronize()
    for k in ("u", "v_hint"):
        assert torch.isfinite(want[k]).all()
        assert torch.equal(got[k], want[k]) and torch.equal(built[k], want[k]), k


# ---- 7. the pipeline --------------------------------------------------------------------------------------------------

def test_dual_pipeline_predict_ragged_and_solve_many_against_per_instance_calls_and_the_solver_oracle():
    from gnn.dual_gnn import DualGNN
    from gnn.features import graph_features_device
    from gnn.pipeline import DualWarmStartPipeline
    from oracle import jv
    from solvers.generators import mixed_batch
    sizes = (96, 64, 33, 1)
    mats, fams = [], []
    for k, n in enumerate(sizes):  # costs within [0, 100]: the unstabilised entropy is not defined beyond
        C, fam = mixed_batch(1, n, families=(("uniform", "clustered")[k % 2],), seed=70 + k)
        mats.append(np.ascontiguousarray(C[0]))
        fams.append(fam[0])
        assert mats[-1].min() >= 0.0 and mats[-1].max() <= 100.0
    assert set(fams) == {"uniform", "clustered"}
    torch.manual_seed(0)
    model = DualGNN(hidden_dim=64, layers=2, heads=4).eval()
    pipe = DualWarmStartPipeline(model, DEV)
    pred = pipe.predict_ragged(mats)
    sol = pipe.solve_many(mats)
    torch.cuda.synchronize()
    assert len(pred) == len(sol) == len(sizes)
    # the references: the CPU fp64 forward of the same weights on each instance's device features, and the
    # unchanged per-instance predict_batch
    feats, alone = [], []
    for C in mats:
        Cd = torch.from_numpy(C).to(DEV)
        feats.append(tuple(t.cpu().double()[None] for t in graph_features_device(Cd)))
        alone.append(pipe.predict_batch(Cd[None])[0][0].cpu().double().numpy())
    model64 = DualGNN(hidden_dim=64, layers=2, heads=4).eval().double()
    model64.load_state_dict({k: v.detach().cpu().double() for k, v in pipe.model.state_dict().items()})
    with torch.no_grad():
        u64 = [model64(*f)["u"][0].numpy() for f in feats]
    for b, (C, n) in enumerate(zip(mats, sizes)):
        u, v = (t.cpu().numpy() for t in pred[b])
        assert u.dtype == np.float64 and v.dtype == np.float64 and u.shape == v.shape == (n,)
        dev_alone = np.abs(alone[b] - u64[b]).max()
        err = np.abs(u - u64[b]).max()
        bound = dg.bound_from(dev_alone)
        print(f"n={n} {fams[b]}: |u_ragged - u64| {err:.3e}, |u_alone - u64| {dev_alone:.3e}, bound {bound:.3e}")
        assert err <= bound, (b, n)
        assert np.array_equal(v, (C - u[:, None]).min(axis=0)), b
        o = sol[b]
        us, vs = o["u"].cpu().numpy(), o["v"].cpu().numpy()
        assert np.array_equal(us, u) and np.array_equal(vs, v), b  # solve_many predicts what predict_ragged does
        r, xo, yo, _ = jv.seeded_raw(C, us, vs)
        assert r == int(o["ret"]), (b, r, int(o["ret"]))
        if r == 0:
            assert np.array_equal(xo, o["x"].cpu().numpy()) and np.array_equal(yo, o["y"].cpu().numpy()), b
