"""Ragged batches on the MI355X: lapwarm_colmin_ragged and lapwarm_row_features_ragged (csrc/ragged_batch.hip and
the ragged instantiation of the row body in csrc/dense_sweeps.hip) through gnn.features, gnn.collate_device and
WarmStartPipeline.predict_ragged / solve_many.

The row body is the uniform kernel's code at n = n_b and a minimum does not depend on the order it is taken in,
so features, top-16 and column minima are compared for equality (NaN where the other has NaN), not within a
tolerance.  Sizes: 1 (the n >= 2 branches), 15 / 16 / 17 (top-k padding), odd and even (median, LDS padding),
255 / 256 / 257 (one element per thread), 513 (more than two per thread)."""
import ctypes as ct
import functools

import numpy as np
import pytest

from dense_sweeps_common import same
from host_common import padded

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 15, 16, 17, 64, 255, 256, 257, 513]
N = max(SIZES)
FAMILIES = ("uniform", "integer", "constant", "wide")
LAYOUTS = ("packed", "padded")


@functools.lru_cache(maxsize=None)
def instances(family):
    """One matrix per size.  integer: 0..9, for ties, column-best counts and all-equal buckets; wide: exp of a
    uniform sample over [0, 40], rows that take the element-wise entropy pass."""
    rs = np.random.RandomState([FAMILIES.index(family), 20])
    out = []
    for n in SIZES:
        if family == "uniform":
            C = rs.uniform(0.0, 1.0, (n, n))
        elif family == "integer":
            C = rs.randint(0, 10, (n, n)).astype(np.float64)
        elif family == "constant":
            C = np.full((n, n), 0.75)
        else:
            C = np.exp(rs.uniform(0.0, 40.0, (n, n)))
        C.setflags(write=False)
        out.append(C)
    return tuple(out)


def pack(mats, layout):
    from gnn.features import ragged_pack
    if layout == "packed":
        p = ragged_pack(list(mats))
        bases = [p.C.data_ptr() + 8 * o for o in p.offsets.tolist()]
        assert p.ld == 0 and any(a % 16 for a in bases) and all(a % 8 == 0 for a in bases)
        return p
    # padded514: an even row stride, so every instance is on the 16-byte path and the odd sizes end in a
    # lane's first column
    width = 514 if layout == "padded514" else N
    p = ragged_pack(padded(mats, width), sizes=[m.shape[0] for m in mats])
    assert p.ld == width and p.N == width and (p.C.data_ptr() % 16 == 0 or width == N)
    return p


@functools.lru_cache(maxsize=None)
def uniform_features_reference(family):
    """row_features_device of every instance alone: computed once, shared, never modified."""
    import torch

    from gnn.features import row_features_device
    out = []
    for C in instances(family):
        feat, topk = row_features_device(torch.from_numpy(C).cuda())
        out.append((feat.cpu().numpy(), topk.cpu().numpy()))
    return out


def raw_call(p, sizes=None, outputs=None, stream=None):
    """lapwarm_row_features_ragged through ctypes into outputs prefilled with NaN (0xFF for the mask and ret);
    `sizes` replaces the pack's device sizes.  Returns the device tensors."""
    import torch

    from lap import _hip
    lib = _hip.require_device()
    dev, B = p.C.device, len(p.host_sizes)
    if outputs is None:
        outputs = dict(feat=torch.full((B, p.N, 21), np.nan, dtype=torch.float32, device=dev),
                       topk=torch.full((B, p.N, 16), np.nan, dtype=torch.float32, device=dev),
                       cost32=torch.full((B, p.N, p.N), np.nan, dtype=torch.float32, device=dev),
                       mask=torch.full((B, p.N), 0xFF, dtype=torch.uint8, device=dev),
                       ret=torch.full((B,), -1, dtype=torch.int32, device=dev))
        nbytes = int(lib.lapwarm_ragged_workspace_bytes(B, p.N))
        assert nbytes >= 8 * B * p.N
        outputs["ws"] = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    o = outputs
    sz = p.sizes if sizes is None else torch.tensor(sizes, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev) if stream is None else stream
    rc = lib.lapwarm_row_features_ragged(p.C.data_ptr(), p.offsets.data_ptr(), sz.data_ptr(), p.ld, B, p.N,
                                         p.posenc.data_ptr(), p.pos_off.data_ptr(), o["feat"].data_ptr(),
                                         o["topk"].data_ptr(), o["cost32"].data_ptr(), o["mask"].data_ptr(),
                                         o["ret"].data_ptr(), o["ws"].data_ptr(), o["ws"].numel(),
                                         ct.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, _hip.last_error())
    return o


def to_host(o):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items() if k != "ws"}


def check_padding(h, sizes, mats):
    """Every word outside the prefixes holds its padding value, cost32 and mask their prefix."""
    for b, n in enumerate(sizes):
        assert (h["feat"][b, n:] == 0).all()
        assert np.isposinf(h["topk"][b, n:]).all() and np.isposinf(h["topk"][b, :n, min(n, 16):]).all()
        want = np.zeros((N, N), dtype=np.float32)
        if n:
            want[:n, :n] = mats[b].astype(np.float32)
        assert same(h["cost32"][b], want), b
        assert h["mask"][b].tolist() == [1] * n + [0] * (N - n)


# ------------------------------------------------------------------------------------------- features
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", FAMILIES)
def test_prefix_is_bit_equal_to_the_uniform_kernel(family, layout):
    from gnn.features import row_features_packed
    mats = instances(family)
    r = row_features_packed(pack(mats, layout), return_topk=True, want_cost32=False)
    feat, topk = r.feat.cpu().numpy(), r.topk.cpu().numpy()
    assert (r.ret.cpu().numpy() == 0).all() and r.sizes.cpu().tolist() == SIZES
    assert r.mask.cpu().numpy().dtype == np.bool_ and r.mask.cpu().numpy().sum(1).tolist() == SIZES
    for b, (n, (f1, t1)) in enumerate(zip(SIZES, uniform_features_reference(family))):
        assert same(feat[b, :n], f1), (family, layout, n, np.argwhere(feat[b, :n] != f1)[:4])
        assert same(topk[b, :n], t1), (family, layout, n)
        assert (feat[b, n:] == 0).all() and np.isposinf(topk[b, n:]).all()


def test_reference_fixtures_in_one_call(features_cases):
    from gnn.features import row_features_ragged
    z = features_cases
    keys = [str(s) for s in z["labels"]]
    r = row_features_ragged([z[f"C__{k}"] for k in keys], return_topk=False)
    feat = r.feat.cpu().numpy()
    assert feat.shape[1] == max(z[f"C__{k}"].shape[0] for k in keys)
    for b, k in enumerate(keys):
        want = z[f"feat__{k}"]
        np.testing.assert_allclose(feat[b, :want.shape[0]], want, rtol=3e-6, atol=1e-9, err_msg=k)
        assert (feat[b, want.shape[0]:] == 0).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_word_of_every_output_is_written(layout):
    mats = instances("uniform")
    h = to_host(raw_call(pack(mats, layout)))
    assert (h["ret"] == 0).all()
    check_padding(h, SIZES, mats)
    for b, (n, (f1, t1)) in enumerate(zip(SIZES, uniform_features_reference("uniform"))):
        assert same(h["feat"][b, :n], f1) and same(h["topk"][b, :n], t1)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bad_sizes_are_reported_and_leave_the_neighbours_alone(layout):
    mats = instances("uniform")
    p = pack(mats, layout)
    good = to_host(raw_call(p))
    sizes = list(SIZES)
    sizes[3], sizes[8] = 0, N + 1  # through the raw entry: the wrappers would refuse them
    h = to_host(raw_call(p, sizes=sizes))
    assert h["ret"].tolist() == [2 if b in (3, 8) else 0 for b in range(len(SIZES))]
    seen = [0 if b in (3, 8) else n for b, n in enumerate(SIZES)]
    check_padding(h, seen, mats)
    for b in range(len(SIZES)):
        if b not in (3, 8):
            for key in ("feat", "topk", "cost32", "mask"):
                assert same(h[key][b], good[key][b]), (key, b)


def test_abi_argument_errors():
    from lap import _hip
    lib = _hip.require_device()
    p = pack(instances("uniform")[:3], "packed")
    o = raw_call(p)
    B = 3

    def call(batch=B, n_pad=p.N, ld=0, C=p.C.data_ptr(), ws_bytes=o["ws"].numel()):
        return lib.lapwarm_row_features_ragged(C, p.offsets.data_ptr(), p.sizes.data_ptr(), ld, batch, n_pad,
                                               p.posenc.data_ptr(), p.pos_off.data_ptr(), o["feat"].data_ptr(),
                                               o["topk"].data_ptr(), None, None, o["ret"].data_ptr(),
                                               o["ws"].data_ptr(), ws_bytes, None)
    assert call(batch=0) == -2 and call(batch=65536) == -2 and call(n_pad=0) == -2 and call(ld=-1) == -2
    assert call(C=None) == -2
    assert call(n_pad=16385) == -5
    assert call(ws_bytes=8) == -1
    assert lib.lapwarm_colmin_ragged(p.C.data_ptr(), p.offsets.data_ptr(), p.sizes.data_ptr(), 0, B, p.N, None,
                                     None, o["ws"].data_ptr(), o["ws"].numel(), None) == -2


# -------------------------------------------------------------------------------------- column minima
@pytest.mark.parametrize("with_u", (False, True), ids=("plain", "minus_u"))
@pytest.mark.parametrize("layout", LAYOUTS + ("padded514",))
def test_colmin_ragged_is_numpy_min(layout, with_u):
    import torch

    from gnn.features import min_trick_ragged
    mats = [m.copy() for m in instances("uniform")]
    mats[6][5, 9] = np.nan   # n = 64: column 9 is NaN, as np.min has it
    mats[10][512, 512] = np.nan
    rs = np.random.RandomState(21)
    p = pack(mats, layout)
    u = np.zeros((len(mats), p.N))
    for b, n in enumerate(SIZES):
        u[b, :n] = rs.normal(0.0, 0.5, n)
    got = min_trick_ragged(p, torch.from_numpy(u).cuda() if with_u else None).cpu().numpy()
    for b, (n, C) in enumerate(zip(SIZES, mats)):
        with np.errstate(invalid="ignore"):
            want = np.min(C - u[b, :n, None], axis=0) if with_u else np.min(C, axis=0)
        assert same(got[b, :n], want), (layout, with_u, n)
        assert (got[b, n:] == 0).all()
    assert np.isnan(got[6, 9]) and np.isnan(got[10, 512]) and np.isnan(got).sum() == 2


# ------------------------------------------------------------------------------------------ consumers
CONSUMER_SIZES = [17, 64, 5, 64, 33]


@functools.lru_cache(maxsize=None)
def consumer_items():
    rs = np.random.RandomState(22)
    return tuple({"cost": rs.uniform(0.0, 1.0, (n, n)), "u": rs.normal(0.0, 0.1, n), "v": rs.normal(0.0, 0.1, n),
                  "n": n} for n in CONSUMER_SIZES)


def model_on_device():
    import torch

    from gnn import OneGNN
    torch.manual_seed(0)
    return OneGNN(21, 64, 2).cuda().eval()


def test_collate_device_fields_and_onegnn_forward():
    """u of the padded batch against the same model on every instance alone, at the project's 1e-5 for the
    forward.  OneGNN.forward subtracts the mean of u over the padded width, masked rows included (the
    reference's forward does, gnn/one_gnn.py:112, and tests/test_gpu_dense_sweeps.py pins it), so an instance
    shorter than the batch maximum comes out shifted by one constant; instances of the full width are compared
    as they are, the shorter ones after their own mean is taken off, which is what the model subtracts when
    the instance is alone."""
    import torch

    from gnn import collate_device
    items = consumer_items()
    model = model_on_device()
    Nc = max(CONSUMER_SIZES)
    bt = collate_device(items)
    assert bt.cost.dtype == torch.float32 and tuple(bt.cost.shape) == (len(items), Nc, Nc)
    assert bt.mask.dtype == torch.bool and bt.sizes.cpu().tolist() == CONSUMER_SIZES
    assert tuple(bt.row_feat.shape) == (len(items), Nc, 21) and tuple(bt.topk.shape) == (len(items), Nc, 16)
    with torch.no_grad():
        u = model(bt.row_feat, topk_values=bt.topk, mask=bt.mask)["u"].cpu().numpy()
    for b, it in enumerate(items):
        n = it["n"]
        assert np.array_equal(bt.cost[b, :n, :n].cpu().numpy(), it["cost"].astype(np.float32))
        assert np.array_equal(bt.u[b, :n].cpu().numpy(), it["u"].astype(np.float32))
        assert np.array_equal(bt.v[b, :n].cpu().numpy(), it["v"].astype(np.float32))
        assert (bt.cost[b, n:] == 0).all() and (bt.cost[b, :, n:] == 0).all()
        assert (bt.u[b, n:] == 0).all() and (bt.v[b, n:] == 0).all()
        assert bt.mask[b].cpu().tolist() == [True] * n + [False] * (Nc - n)
        one = collate_device([it])
        with torch.no_grad():
            alone = model(one.row_feat, topk_values=one.topk, mask=one.mask)["u"][0].cpu().numpy()
        mine = u[b, :n] if n == Nc else u[b, :n] - u[b, :n].astype(np.float64).mean()
        err = np.abs(mine - alone).max()
        print(f"instance {b} n={n}: max |u - alone| = {err:.3g}")
        assert err <= 1e-5, (b, n, err)
        assert (u[b, n:] == 0).all()


def test_one_training_step_on_a_collated_batch():
    import torch

    from gnn import collate_device
    from gnn.losses import warmstart_loss
    bt = collate_device(consumer_items())
    model = model_on_device().train()
    model.fused_refine_training = True
    u = model(bt.row_feat, topk_values=bt.topk, mask=bt.mask)["u"]
    loss, metrics = warmstart_loss(bt.cost, u, bt.u, bt.mask)
    loss.backward()
    assert torch.isfinite(loss).item() and (metrics["ret"] == 0).all()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name


def test_predict_ragged_matches_the_predictor_per_instance():
    from gnn import GNNPredictor, WarmStartPipeline
    model = model_on_device()
    costs = [it["cost"] for it in consumer_items()]
    got = WarmStartPipeline(model).predict_ragged(costs)
    one = GNNPredictor(model=model)
    assert len(got) == len(costs)
    for C, (u_hat, v_hat) in zip(costs, got):
        u_hat, v_hat = u_hat.cpu().numpy(), v_hat.cpu().numpy()
        assert u_hat.dtype == np.float64 and v_hat.dtype == np.float64 and u_hat.shape == (C.shape[0],)
        u_ref, _ = one.predict(C)
        err = np.abs(u_hat - u_ref).max()
        print(f"n={C.shape[0]}: max |u_hat - predict| = {err:.3g}")
        assert err <= 1e-5
        assert same(v_hat, np.min(C - u_hat[:, None], axis=0))


def test_solve_many_groups_by_size_and_keeps_the_input_order():
    import torch

    from gnn import WarmStartPipeline
    sizes = [64, 17, 64, 256]
    rs = np.random.RandomState(23)
    costs = [rs.uniform(0.0, 1.0, (n, n)) for n in sizes]
    pipe = WarmStartPipeline(model_on_device())
    got = pipe.solve_many(costs)
    assert [g["x"].shape[0] for g in got] == sizes
    for n in sorted(set(sizes)):
        members = [b for b, m in enumerate(sizes) if m == n]
        ref = pipe.solve_batch(torch.from_numpy(np.stack([costs[b] for b in members])).cuda())
        for k, b in enumerate(members):
            for key in ("x", "y", "ret"):
                assert torch.equal(got[b][key], ref[key][k]), (key, b)
            assert (got[b]["u"] - ref["u"][k]).abs().max().item() <= 1e-5
            x = got[b]["x"].cpu().numpy()
            assert got[b]["ret"].item() != 0 or sorted(x.tolist()) == list(range(n))


# -------------------------------------------------------------------------------------- graph capture
def test_graph_replay_rewrites_poisoned_outputs():
    import torch
    p = pack(instances("integer"), "packed")
    eager = to_host(raw_call(p))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        o = raw_call(p, stream=s)  # warm-up on the side stream; these buffers are the graph's
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one stream, no parallel branches
        raw_call(p, outputs=o)
    for key, t in o.items():
        t.fill_(0xFF) if t.dtype in (torch.uint8, torch.int32) else t.fill_(float("nan"))
    g.replay()
    got = to_host(o)
    for key in eager:
        assert same(got[key], eager[key]), key
