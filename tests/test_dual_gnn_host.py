"""DualGNN without a GPU: the module against the reference's recorded outputs (plain torch path), the folding
against the plain path in fp64, the ABI surface of the new entries, the workspace queries, the checkpoint
loader and the public names."""
import numpy as np
import pytest
import torch

import dual_gnn_common as dg
from host_common import lib  # noqa: F401


@pytest.mark.parametrize("cfg", dg.cfg_labels())
def test_state_dict_names_shapes_and_parameter_count_equal_the_reference(cfg):
    from gnn.dual_gnn import DualGNN
    hidden, heads, layers, count = (int(v) for v in dg.cases()[f"cfg/{cfg}"])
    model = DualGNN(hidden_dim=hidden, layers=layers, heads=heads)
    want = dg.state_dict(cfg)
    got = model.state_dict()
    assert list(got) == list(want)
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in want.items()}
    assert sum(p.numel() for p in model.parameters()) == count
    assert count == {"h32_H4_L2": 62418, "h128_H4_L1": 171658}.get(cfg, count)


@pytest.mark.parametrize("label", dg.model_labels())
def test_plain_path_on_cpu_reproduces_the_reference_float32_outputs(label):
    z = dg.cases()
    model = dg.build_model(label.split("@")[0])
    edge, row, col, mask = dg.model_inputs(label)
    with torch.no_grad():
        out = model(edge, row, col, mask)
    bound = dg.model_bound(label)
    du = np.abs(out["u"].numpy() - z[f"out/{label}/u32"]).max()
    dv = np.abs(out["v_hint"].numpy() - z[f"out/{label}/v32"]).max()
    print(f"{label}: |u - u32| {du:.3e}, |v - v32| {dv:.3e}, bound 4 x max|u32 - u64| = {bound:.3e}")
    assert set(out) == {"u", "v_hint"} and out["u"].dtype == torch.float32
    assert du <= bound and dv <= bound


@pytest.mark.parametrize("label", dg.model_labels())
def test_folded_formulation_equals_the_plain_path_in_fp64(label):
    z = dg.cases()
    model = dg.build_model(label.split("@")[0], torch.float64)
    edge, row, col, mask = dg.model_inputs(label)
    edge, row, col = edge.double(), row.double(), col.double()
    with torch.no_grad():
        plain = model(edge, row, col, mask)
    u, v = dg.folded_forward(model, edge, row, col, mask)
    assert (u - plain["u"]).abs().max().item() <= 1e-12
    assert (v - plain["v_hint"]).abs().max().item() <= 1e-12
    # and the plain fp64 path is the reference's fp64 forward
    assert np.abs(plain["u"].numpy() - z[f"out/{label}/u64"]).max() <= 1e-12
    assert np.abs(plain["v_hint"].numpy() - z[f"out/{label}/v64"]).max() <= 1e-12


@pytest.mark.parametrize("label", dg.feat_labels())
def test_features_numpy_equals_the_reference_recorded_features_bit_for_bit(label):
    """What lets the GPU tests use features_numpy as their reference at sizes the fixture does not hold.  The tied
    case's rank channels are excluded: the recorded ranking comes from an unstable argsort and is one valid
    ranking among several; features_numpy's must be the stable one."""
    z = dg.cases()
    C = z[f"feat/{label}/C"]
    key = f"feat/{label}/u"
    edge, row, col = dg.features_numpy(C, z[key] if key in z.files else None)
    want = {k: z[f"feat/{label}/{k}"] for k in ("edge", "row", "col")}
    assert edge.dtype == np.float32 and row.dtype == np.float32 and col.dtype == np.float32
    assert np.array_equal(row, want["row"]) and np.array_equal(col, want["col"])
    tied = label.startswith("ties")
    assert edge.shape == want["edge"].shape
    for ch in range(10):
        if tied and ch in (1, 2):
            continue
        assert np.array_equal(edge[..., ch], want["edge"][..., ch]), (label, ch)
    n = C.shape[0]
    dg.assert_valid_stable_ranks(C, dg.integer_ranks(edge[..., 1], n))
    dg.assert_valid_stable_ranks(C.T, dg.integer_ranks(edge[..., 2], n).T)


def test_features_numpy_batches_like_single_calls_and_ranks_signed_zeros_by_index():
    rng = np.random.default_rng(3)
    C = rng.random((2, 6, 6)) - 0.5
    C[0, 0, :5] = [0.0, -0.0, 0.0, -0.0, 0.0]
    u = rng.random((2, 6))
    both = dg.features_numpy(C, u)
    for b in range(2):
        for got, one in zip(both, dg.features_numpy(C[b], u[b])):
            assert np.array_equal(got[b], one)
    ranks = dg.integer_ranks(both[0][0, 0, :, 1], 6)
    zeros_first = int((C[0, 0] < 0).sum())
    assert ranks[:5].tolist() == list(range(zeros_first, zeros_first + 5))


def test_training_mode_and_gradients_take_the_plain_path():
    model = dg.build_model("h32_H4_L2")
    edge, row, col, mask = dg.model_inputs("h32_H4_L2@pad")
    assert not model.layers[0].takes_fused_path(edge, row, col)  # CPU tensors
    out = model(edge, row, col, mask)  # gradient recorded
    out["u"].sum().backward()
    assert model.layers[0].edge_mlp[5].weight.grad is not None
    model.train()
    torch.manual_seed(0)
    a = model(edge, row, col, mask)["u"]
    b = model(edge, row, col, mask)["u"]
    assert not torch.equal(a, b)  # dropout is active


def test_workspace_queries_are_monotone_and_refuse_bad_arguments(lib):
    q = lib.lapwarm_dual_gnn_workspace_bytes
    assert q(0, 8, 4) == 0 and q(1, 0, 4) == 0 and q(1, 8, 0) == 0 and q(1, 8, 9) == 0 and q(1, 16385, 4) == 0
    assert q(1, 1, 1) >= 8 and q(3, 40, 4) >= 3 * 2 * 4 * 40 * 40 * 4
    sizes = [q(B, N, 4) for B in (1, 2, 5) for N in (7, 64, 65, 300)]
    assert all(s > 0 for s in sizes)
    for N in (7, 64, 65, 300):
        assert q(1, N, 4) <= q(2, N, 4) <= q(5, N, 4)
    for B in (1, 2, 5):
        assert q(B, 7, 4) <= q(B, 64, 4) < q(B, 65, 4) < q(B, 300, 4)
    assert q(1, 1024, 4) >= 2 * 4 * 1024 * 1024 * 4
    g = lib.lapwarm_graph_features_workspace_bytes
    assert g(0, 8) == 0 and g(1, 0) == 0 and g(1, 4097) == 0 and g(32768, 8) == 0
    assert 0 < g(1, 1) <= g(1, 2) <= g(1, 17) < g(1, 64) < g(1, 65) < g(2, 65) < g(2, 4096)
    assert g(2, 65) >= 2 * 65 * 65 * (8 + 2 * 4)  # the transposed copy and the two rank planes


def test_argument_errors_return_before_any_device_work(lib):
    dev = 1 << 20  # never dereferenced
    ws = lib.lapwarm_graph_features_workspace_bytes(2, 17)
    gf = lib.lapwarm_graph_features_batched
    assert gf(dev, 0, 17, None, dev, dev, dev, dev, dev, ws, None) == -2
    assert gf(dev, 2, 0, None, dev, dev, dev, dev, dev, ws, None) == -2
    assert gf(dev, 2, 4097, None, dev, dev, dev, dev, dev, ws, None) == -5
    assert gf(None, 2, 17, None, dev, dev, dev, dev, dev, ws, None) == -2
    assert gf(dev, 2, 17, None, dev, dev, dev, dev, dev, ws - 1, None) == -1
    es = lib.lapwarm_dual_edge_scores
    assert es(dev, dev, dev, dev, dev, dev, dev, 1, 8, 9, None) == -2   # heads > 8
    assert es(dev, dev, dev, dev, dev, dev, dev, 1, 8, 0, None) == -2
    assert es(dev, dev, dev, dev, dev, dev, None, 1, 8, 4, None) == -2
    assert es(dev, dev, dev, dev, dev, dev, dev, 1, 16385, 4, None) == -5
    at = lib.lapwarm_dual_attention
    assert at(dev, dev, dev, dev, dev, dev, None, dev, dev, dev, dev, 0, 8, 4, 8, None) == -2
    assert at(dev, dev, dev, dev, dev, dev, None, dev, dev, dev, None, 1, 8, 4, 8, None) == -2
    assert at(dev, dev, dev, dev, dev, dev, None, dev, dev, dev, dev, 1, 8, 4, 0, None) == -2


def test_load_dual_checkpoint_handles_the_three_schemas(tmp_path):
    import gnn
    from gnn.dual_gnn import DualGNN
    torch.manual_seed(3)
    default = DualGNN()
    torch.save(default.state_dict(), tmp_path / "bare.pt")
    model, info = gnn.load_dual_checkpoint(tmp_path / "bare.pt", "cpu")
    assert (info["hidden_dim"], info["layers"], info["heads"], info["dropout"]) == (128, 4, 4, 0.1)
    assert not model.training and len(model.layers) == 4 and model.layers[0].heads == 4
    for k, v in default.state_dict().items():
        assert torch.equal(model.state_dict()[k], v)
    small = DualGNN(hidden_dim=48, layers=2, heads=8, dropout=0.0)
    flat = {"model_state_dict": small.state_dict(), "architecture": "dual_gnn", "hidden_dim": 48, "layers": 2,
            "heads": 8, "dropout": 0.0}
    nested = {"model_state_dict": small.state_dict(),
              "config": {"architecture": "dual_gnn", "hidden_dim": 48, "layers": 2, "heads": 8, "dropout": 0.0}}
    for name, ck in (("flat.pt", flat), ("nested.pt", nested)):
        torch.save(ck, tmp_path / name)
        model, info = gnn.load_dual_checkpoint(tmp_path / name, "cpu")
        assert (info["hidden_dim"], info["layers"], info["heads"]) == (48, 2, 8)
        assert model.layers[1].heads == 8 and model.layers[1].head_dim == 6
        for k, v in small.state_dict().items():
            assert torch.equal(model.state_dict()[k], v)
    torch.save({"model_state_dict": small.state_dict(), "architecture": "one_gnn"}, tmp_path / "one.pt")
    with pytest.raises(ValueError, match="one_gnn"):
        gnn.load_dual_checkpoint(tmp_path / "one.pt", "cpu")


def test_real_names_are_reachable_while_the_pinned_names_still_raise():
    import gnn
    import gnn.dual_gnn
    import gnn.features
    import gnn.pipeline
    model = gnn.dual_gnn.DualGNN(hidden_dim=16, layers=1, heads=2)
    assert isinstance(model.layers[0], gnn.dual_gnn.DualLayer)
    assert gnn.DualGNN is not gnn.dual_gnn.DualGNN and gnn.compute_features is not gnn.features.compute_features
    with pytest.raises(NotImplementedError, match="DualGNN"):
        gnn.DualGNN(hidden_dim=16)
    with pytest.raises(NotImplementedError, match="compute_features"):
        gnn.compute_features(np.zeros((2, 2)))
    assert callable(gnn.features.graph_features_device) and callable(gnn.load_dual_checkpoint)
    assert (gnn.features.EDGE_FEATURE_DIM, gnn.features.NODE_FEATURE_DIM) == (10, 14)
    assert issubclass(gnn.pipeline.DualWarmStartPipeline, gnn.WarmStartPipeline)
    own = {k for k, v in vars(gnn.pipeline.DualWarmStartPipeline).items() if callable(v)}
    assert own == {"predict_batch"}
    assert "load_dual_checkpoint" in gnn.__doc__ and "run_harness.py" in gnn.__doc__
    with pytest.raises(RuntimeError, match="MI355X"):
        gnn.pipeline.DualGNNPredictor(model=model, device="cpu")
