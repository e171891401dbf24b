"""DualGNN on the MI355X: graph features against the reference's recorded ones, the two kernels of the fused
attention against fp64 torch, the fused forward against the reference's fp64 outputs and against the plain path,
and the DualGNN warm-start pipeline against the CPU solver oracle.

Bounds against fp64 are dual_gnn_common.bound_from: 4 x the deviation of a float32 CPU evaluation of the same
expression (for the model: the reference's own max|u32 - u64| on the case, recorded in the fixture, for u and
for v_hint alike), never looser than 1e-5."""
import ctypes as ct

import numpy as np
import pytest
import torch

import dual_gnn_common as dg
from host_common import device_lib as lib  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _stream():
    return ct.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


# ---- features ------------------------------------------------------------------------------------------------

def _device_features(label):
    from gnn.features import graph_features_device
    z = dg.cases()
    C = torch.from_numpy(z[f"feat/{label}/C"]).to(DEV)
    key = f"feat/{label}/u"
    u = torch.from_numpy(z[key]).to(DEV) if key in z.files else None
    edge, row, col = graph_features_device(C, u)
    torch.cuda.synchronize()
    return edge.cpu().numpy(), row.cpu().numpy(), col.cpu().numpy()


@pytest.mark.parametrize("label", dg.feat_labels())
def test_graph_features_against_the_reference(label):
    z = dg.cases()
    C = z[f"feat/{label}/C"]
    n = C.shape[0]
    edge, row, col = _device_features(label)
    want = {k: z[f"feat/{label}/{k}"] for k in ("edge", "row", "col")}
    assert edge.shape == (n, n, 10) and row.shape == (n, 14) and col.shape == (n, 14)
    tied = label.startswith("ties")
    for ch in range(10):
        if tied and ch in (1, 2):
            continue
        assert np.allclose(edge[..., ch], want["edge"][..., ch], rtol=2e-6, atol=1e-9), (label, ch)
    for ch in range(14):
        assert np.allclose(row[:, ch], want["row"][:, ch], rtol=2e-6, atol=1e-9), (label, "row", ch)
        assert np.allclose(col[:, ch], want["col"][:, ch], rtol=2e-6, atol=1e-9), (label, "col", ch)
    d = max(1, n - 1)
    rr = np.rint(edge[..., 1].astype(np.float64) * d).astype(np.int64)
    cr = np.rint(edge[..., 2].astype(np.float64) * d).astype(np.int64)
    # a rank is exactly k / (n - 1) rounded to float32 (0 at n = 1)
    assert np.array_equal((rr / d).astype(np.float32), edge[..., 1] if n > 1 else np.zeros_like(edge[..., 1]))
    assert np.array_equal((cr / d).astype(np.float32), edge[..., 2] if n > 1 else np.zeros_like(edge[..., 2]))
    if tied:
        dg.assert_valid_stable_ranks(C, rr)
        dg.assert_valid_stable_ranks(C.T, cr.T)
    else:
        assert np.array_equal(rr, np.rint(want["edge"][..., 1].astype(np.float64) * d).astype(np.int64))
        assert np.array_equal(cr, np.rint(want["edge"][..., 2].astype(np.float64) * d).astype(np.int64))
    if label.startswith("const_row"):
        assert row[4, 4] == np.float32(1e-9)  # the MAD floor
    if not label.startswith("reduced"):
        assert not edge[..., 9].any()


def test_graph_features_batched_equal_single_and_compute_features_wraps_them():
    from gnn.features import GraphFeatures, compute_features, graph_features_device
    z = dg.cases()
    C = np.stack([z["feat/uniform_n65/C"], z["feat/uniform_n65/C"].T.copy()])
    edge, row, col = graph_features_device(torch.from_numpy(C).to(DEV))
    one = _device_features("uniform_n65")
    assert np.array_equal(edge[0].cpu().numpy(), one[0]) and np.array_equal(row[0].cpu().numpy(), one[1])
    assert np.array_equal(col[1].cpu().numpy(), one[1])  # the transposed instance: columns are the rows
    f = compute_features(z["feat/reduced_n17/C"], include_reduced_cost=True, u=z["feat/reduced_n17/u"])
    assert isinstance(f, GraphFeatures) and f.edge_feat.dtype == np.float32
    assert np.array_equal(f.edge_feat, _device_features("reduced_n17")[0])


# ---- lapwarm_dual_edge_scores ---------------------------------------------------------------------------------

def _edge_score_case(B, N, heads):
    g = torch.Generator().manual_seed(1000 * N + heads)
    edge = torch.rand((B, N, N, 10), generator=g) * 2.0 - 0.5
    W1 = (torch.rand((128, 10), generator=g) - 0.5) * 0.6
    b1 = (torch.rand((128,), generator=g) - 0.5) * 0.2
    W2 = (torch.rand((128, 128), generator=g) - 0.5) * 0.18
    b2 = (torch.rand((128,), generator=g) - 0.5) * 0.2
    G = (torch.rand((2 * heads, 128), generator=g) - 0.5) * 0.3
    return edge, W1, b1, W2, b2, G


def _launch_edge_scores(lib, d, out_ptr, B, N, heads):
    """d: the six arguments on the device, contiguous"""
    rc = lib.lapwarm_dual_edge_scores(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                      d[4].data_ptr(), d[5].data_ptr(), out_ptr, B, N, heads, _stream())
    torch.cuda.synchronize()
    assert rc == 0


def _check_edge_scores(lib, B, N, heads):
    args = _edge_score_case(B, N, heads)
    want = dg.edge_scores_torch(*(a.double() for a in args))
    dev32 = (dg.edge_scores_torch(*args).double() - want).abs().max().item()
    bound = dg.bound_from(dev32)
    count = B * 2 * heads * N * N
    guard = 64
    poison = float.fromhex("0x1.5p+100")
    buf = torch.full((count + 2 * guard,), poison, dtype=torch.float32, device=DEV)
    d = [a.to(DEV).contiguous() for a in args]
    _launch_edge_scores(lib, d, buf[guard:].data_ptr(), B, N, heads)
    out = buf.cpu()
    assert torch.all(out[:guard] == poison) and torch.all(out[guard + count:] == poison)
    got = out[guard:guard + count].reshape(B, 2, heads, N, N).double()
    err = (got - want).abs().max().item()
    print(f"B={B} N={N} heads={heads}: device {err:.3e}, torch fp32 {dev32:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("heads", [1, 4, 8])
@pytest.mark.parametrize("N", [1, 7, 16, 17, 65])
def test_edge_scores_against_fp64_torch_and_nothing_outside_is_written(lib, N, heads):
    _check_edge_scores(lib, 2, N, heads)


# The launch caps the grid at 256 workgroups, each walking tiles of 128 edges with a stride of the grid: (1, 257, 8)
# and (3, 151, 3) are 66 049 and 68 403 edges, 517 and 535 tiles, so every workgroup takes two or three, and the
# second has its two instance boundaries inside tiles.  heads 3 and 5 end 2 * heads inside a lane group of four.
@pytest.mark.parametrize("B,N,heads", [(1, 257, 8), (3, 151, 3), (2, 17, 3), (2, 17, 5)])
def test_edge_scores_past_one_trip_of_the_tile_loop_and_with_odd_head_counts(lib, B, N, heads):
    _check_edge_scores(lib, B, N, heads)


def test_edge_scores_of_a_batch_equal_single_instance_launches_bit_for_bit(lib):
    """An edge's scores depend on its own column of the MFMA tiles only, so neither its place in a tile nor the
    tile's place in the grid may matter: instances 1 and 2 start inside a tile here (22 801 edges each)."""
    B, N, heads = 3, 151, 3
    d = [a.to(DEV).contiguous() for a in _edge_score_case(B, N, heads)]
    count = 2 * heads * N * N
    together = torch.full((B * count,), float("nan"), dtype=torch.float32, device=DEV)
    _launch_edge_scores(lib, d, together.data_ptr(), B, N, heads)
    assert torch.isfinite(together).all()
    for b in range(B):
        alone = torch.full((count,), float("nan"), dtype=torch.float32, device=DEV)
        _launch_edge_scores(lib, [d[0][b:b + 1].contiguous()] + d[1:], alone.data_ptr(), 1, N, heads)
        assert torch.equal(alone, together[b * count:(b + 1) * count]), b


# ---- lapwarm_dual_attention -----------------------------------------------------------------------------------

SCORE_RANGE = 3.0  # the generator's scores are uniform in [-3, 3); a, c and the bias in [-1, 1)


def _attention_case(B, N, H, D, mask, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g) * 2.0 - 1.0  # noqa: E731
    return dict(scores=r(B, 2, H, N, N) * (SCORE_RANGE * scale), a_row=r(B, H, N), c_row=r(B, H, N),
                a_col=r(B, H, N), c_col=r(B, H, N),
                kbias=r(2 * H), mask=mask, row_val=r(B, N, H * D), col_val=r(B, N, H * D))


def _run_attention(lib, case, B, N, H, D):
    d = {k: (v.to(DEV).contiguous() if v is not None else None) for k, v in case.items()}
    m8 = d["mask"].to(torch.uint8) if d["mask"] is not None else None
    row_msg = torch.full((B, N, H * D), float("nan"), dtype=torch.float32, device=DEV)
    col_msg = torch.full((B, N, H * D), float("nan"), dtype=torch.float32, device=DEV)
    rc = lib.lapwarm_dual_attention(d["scores"].data_ptr(), d["a_row"].data_ptr(), d["c_row"].data_ptr(),
                                    d["a_col"].data_ptr(), d["c_col"].data_ptr(), d["kbias"].data_ptr(),
                                    m8.data_ptr() if m8 is not None else None, d["row_val"].data_ptr(),
                                    d["col_val"].data_ptr(), row_msg.data_ptr(), col_msg.data_ptr(), B, N, H, D,
                                    _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return row_msg.cpu(), col_msg.cpu()


def _masks(kind, B, N):
    if kind == "all":
        return torch.ones((B, N), dtype=torch.bool)
    if kind == "none":
        return None
    m = torch.zeros((B, N), dtype=torch.bool)
    sizes = [N, max(1, (2 * N) // 3), 1][:B] if kind == "ragged" else [N, 0, max(1, N // 2)][:B]
    for b, n in enumerate(sizes):
        m[b, :n] = True
    return m


def _check_attention(lib, N, H, D, kind, scale=1.0):
    """-> the fp64 reference's largest |logit| (after the leaky ReLU, over the unmasked pairs)"""
    B = 3
    mask = _masks(kind, B, N)
    case = _attention_case(B, N, H, D, mask, seed=N * 100 + H, scale=scale)
    as64 = {k: (v.double() if v is not None and v.dtype != torch.bool else v) for k, v in case.items()}
    want = dg.attention_torch(**as64)
    ref32 = dg.attention_torch(**case)
    got = _run_attention(lib, case, B, N, H, D)
    again = _run_attention(lib, case, B, N, H, D)
    for a, b, w, r32 in zip(got, again, want, ref32):  # the row messages, then the column messages
        assert torch.equal(a, b)
        assert torch.isfinite(a).all()
        dev32 = (r32.double() - w).abs().max().item()
        bound = dg.bound_from(dev32)
        err = (a.double() - w).abs().max().item()
        print(f"N={N} H={H} D={D} {kind}: device {err:.3e}, torch fp32 {dev32:.3e}, bound {bound:.3e}")
        assert err <= bound
    if mask is not None:
        assert not got[0][~mask].any() and not got[1][~mask].any()  # masked queries: zero messages
    keep = mask if mask is not None else torch.ones((B, N), dtype=torch.bool)
    pair = (keep[:, None, :, None] & keep[:, None, None, :])[:, None]  # (B, 1, 1, N, N) over both directions
    s64, k64 = as64["scores"], as64["kbias"].reshape(1, 2, H, 1, 1)
    pre = torch.stack([as64["a_row"][..., :, None] + as64["c_row"][..., None, :],
                       as64["c_col"][..., :, None] + as64["a_col"][..., None, :]], dim=1) + s64 + k64
    logits = torch.nn.functional.leaky_relu(pre, 0.2)
    return logits.abs().masked_fill(~pair, 0.0).max().item()


@pytest.mark.parametrize("N,H,D,kind", [(70, 4, 8, "all"), (70, 4, 8, "ragged"), (33, 8, 8, "empty"),
                                        (1, 2, 16, "none"), (17, 1, 136, "ragged"), (130, 2, 32, "ragged")])
def test_attention_against_fp64_torch_and_twice_the_same_bits(lib, N, H, D, kind):
    assert _check_attention(lib, N, H, D, kind) < 10.0


def test_attention_with_logits_beyond_100_needs_the_maximum_subtracted(lib):
    """scores uniform in [-150, 150): expf overflows near 88, so a softmax without its maximum subtracted gives inf
    or NaN here, while every other case of this file has logits of at most about 6."""
    largest = _check_attention(lib, 70, 2, 8, "ragged", scale=150.0 / SCORE_RANGE)
    print(f"largest |logit| of the fp64 reference: {largest:.1f}")
    assert largest > 100.0


def test_attention_with_a_head_dimension_below_the_16_slots_and_odd(lib):
    _check_attention(lib, 20, 3, 5, "none")  # hidden = 15


# ---- the whole model ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("label", dg.model_labels())
def test_fused_forward_against_the_reference_fp64_outputs(label):
    z = dg.cases()
    model = dg.build_model(label.split("@")[0]).to(DEV)
    edge, row, col, mask = (t.to(DEV) if t is not None else None for t in dg.model_inputs(label))
    assert model.layers[0].takes_fused_path(edge, row, col) is False  # gradients would be recorded here
    with torch.no_grad():
        assert model.layers[0].takes_fused_path(edge, row, col)
        out = model(edge, row, col, mask)
        with torch.autocast("cuda"):
            cast = model(edge, row, col, mask)
    torch.cuda.synchronize()
    bound = dg.model_bound(label)
    du = np.abs(out["u"].cpu().numpy().astype(np.float64) - z[f"out/{label}/u64"]).max()
    dv = np.abs(out["v_hint"].cpu().numpy().astype(np.float64) - z[f"out/{label}/v64"]).max()
    ref_dv = float(z[f"out/{label}/dv"])
    print(f"{label}: |u - u64| {du:.3e}, |v - v64| {dv:.3e}, bound 4 x max|u32 - u64| = {bound:.3e} "
          f"(the reference's own max|v32 - v64| is {ref_dv:.3e})")
    assert out["u"].dtype == torch.float32 and cast["u"].dtype == torch.float32
    assert torch.equal(out["u"], cast["u"]) and torch.equal(out["v_hint"], cast["v_hint"])  # autocast is ignored
    assert du <= bound and dv <= bound


def test_fused_forward_against_the_plain_path_on_the_device():
    from gnn.dual_gnn import DualGNN
    from gnn.features import graph_features_device
    torch.manual_seed(11)
    model = DualGNN(hidden_dim=128, layers=4, heads=4).eval()
    rng = np.random.default_rng(5)
    C = torch.from_numpy(rng.random((2, 96, 96)) * 10.0).to(DEV)
    edge, row, col = graph_features_device(C)
    with torch.no_grad():
        ref64 = model.double()(edge.cpu().double(), row.cpu().double(), col.cpu().double())
        model = model.float().to(DEV)
        fused = model(edge, row, col)
    plain = model(edge, row, col)  # a gradient is recorded: the plain path
    assert plain["u"].requires_grad and not fused["u"].requires_grad
    torch.cuda.synchronize()
    for k in ("u", "v_hint"):  # each output against 4 x the plain path's own deviation on that output
        dev = (plain[k].detach().cpu().double() - ref64[k]).abs().max().item()
        err = (fused[k].cpu().double() - ref64[k]).abs().max().item()
        bound = dg.bound_from(dev)
        print(f"h128 H4 L4 B=2 n=96 {k}: fused {err:.3e}, plain on the device {dev:.3e}, bound {bound:.3e}")
        assert err <= bound, k


def test_fused_forward_with_a_mask_where_every_kernel_loop_repeats():
    """B = 3, N = 150, sizes (150, 97, 1): 67 500 edges are 528 tiles for at most 256 workgroups, and attention needs
    three key tiles; the masked model cases of the fixture stop at N = 40."""
    from gnn.dual_gnn import DualGNN
    sizes, N = (150, 97, 1), 150
    rng = np.random.default_rng(150)
    edge = np.zeros((len(sizes), N, N, 10), np.float32)
    row = np.zeros((len(sizes), N, 14), np.float32)
    col = np.zeros_like(row)
    mask = torch.zeros((len(sizes), N), dtype=torch.bool)
    for b, n in enumerate(sizes):  # every instance's features at its own size, zero-padded to N
        edge[b, :n, :n], row[b, :n], col[b, :n] = dg.features_numpy(rng.random((n, n)) * 10.0)
        mask[b, :n] = True
    edge, row, col = torch.from_numpy(edge), torch.from_numpy(row), torch.from_numpy(col)
    torch.manual_seed(12)
    model = DualGNN(hidden_dim=64, layers=2, heads=8).eval()
    with torch.no_grad():
        ref64 = model.double()(edge.double(), row.double(), col.double(), mask)
        model = model.float().to(DEV)
        e, r, c, m = edge.to(DEV), row.to(DEV), col.to(DEV), mask.to(DEV)
        assert model.layers[0].takes_fused_path(e, r, c)
        fused = model(e, r, c, m)
    plain = model(e, r, c, m)  # a gradient is recorded: the plain path
    assert plain["u"].requires_grad and not fused["u"].requires_grad
    torch.cuda.synchronize()
    for k in ("u", "v_hint"):  # each output against 4 x the plain path's own deviation on that output
        dev = (plain[k].detach().cpu().double() - ref64[k]).abs().max().item()
        err = (fused[k].cpu().double() - ref64[k]).abs().max().item()
        bound = dg.bound_from(dev)
        print(f"h64 H8 L2 B=3 N=150 masked {k}: fused {err:.3e}, plain on the device {dev:.3e}, bound {bound:.3e}")
        assert err <= bound, k
        assert torch.isfinite(fused[k]).all()
        assert not fused[k].cpu()[~mask].any() and not ref64[k][~mask].any()  # padded slots are exactly 0


# ---- the pipeline ---------------------------------------------------------------------------------------------

def test_dual_pipeline_solve_batch_against_the_solver_oracle():
    from gnn.dual_gnn import DualGNN
    from gnn.pipeline import DualGNNPredictor, DualWarmStartPipeline
    from oracle import jv
    from solvers.generators import mixed_batch
    B, n = 4, 96
    # the families whose costs stay within [0, 100] (sparse holds 1e6 entries, metric exceeds 100): the
    # unstabilised entropy of the graph features is not defined for larger costs
    C_host, fams = mixed_batch(B, n, families=("uniform", "clustered"), seed=7)
    assert C_host.min() >= 0.0 and C_host.max() <= 100.0
    torch.manual_seed(0)
    model = DualGNN(hidden_dim=64, layers=2, heads=4).eval()
    pipe = DualWarmStartPipeline(model, DEV)
    out = pipe.solve_batch(torch.from_numpy(C_host).to(DEV))
    torch.cuda.synchronize()
    x, y, ret = out["x"].cpu().numpy(), out["y"].cpu().numpy(), out["ret"].cpu().numpy()
    u, v = out["u"].cpu().numpy(), out["v"].cpu().numpy()
    assert np.isfinite(u).all() and np.isfinite(v).all() and u.dtype == np.float32 and v.dtype == np.float64
    for b in range(B):
        assert np.array_equal(v[b], (C_host[b] - u[b].astype(np.float64)[:, None]).min(axis=0)), fams[b]
        r, xo, yo, _ = jv.seeded_raw(C_host[b], u[b].astype(np.float64), v[b])
        assert r == ret[b], (fams[b], r, ret[b])
        if r == 0:
            assert np.array_equal(xo, x[b]) and np.array_equal(yo, y[b]), fams[b]
    pu, pv = DualGNNPredictor(model=model).predict(C_host[0])
    assert pu.dtype == np.float64 and np.array_equal(pu, u[0].astype(np.float64)) and np.array_equal(pv, v[0])
