"""DualWarmStartPipeline.dual_training_batch on the MI355X: the labelled DualGNN batch of four instances of different
sizes against the pieces it joins (graph_features_ragged, the float32 cast, the labels of training_batch), and one
training step model -> dual_warmstart_loss -> backward through the fused attention."""
import numpy as np
import pytest

from solvers.generators import mixed_batch

pytestmark = pytest.mark.gpu

SIZES = (5, 33, 64, 130)


@pytest.fixture(scope="module")
def setup():
    import torch

    from gnn.dual_gnn import DualGNN
    from gnn.pipeline import DualWarmStartPipeline
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    mats = [np.ascontiguousarray(mixed_batch(1, n, families=("uniform",), seed=90 + k)[0][0])
            for k, n in enumerate(SIZES)]
    torch.manual_seed(0)
    model = DualGNN(hidden_dim=32, layers=2, heads=4).eval()
    pipe = DualWarmStartPipeline(model, torch.device("cuda:0"))
    return torch, pipe, mats


def test_batch_is_the_pieces_it_joins(setup):
    torch, pipe, mats = setup
    from gnn.collate import DualDeviceBatch
    from gnn.features import graph_features_ragged
    got = pipe.dual_training_batch(mats)
    want = graph_features_ragged(mats, device="cuda:0")
    labels = pipe.training_batch(mats)
    torch.cuda.synchronize()
    N = max(SIZES)
    assert isinstance(got, DualDeviceBatch)
    for name, a, b in (("edge_feat", got.edge_feat, want.edge), ("row_feat", got.row_feat, want.row),
                       ("col_feat", got.col_feat, want.col), ("mask", got.mask, want.mask),
                       ("sizes", got.sizes, want.sizes), ("u", got.u, labels.u), ("v", got.v, labels.v),
                       ("cost", got.cost, labels.cost)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert got.edge_feat.shape == (4, N, N, 10) and got.row_feat.shape == got.col_feat.shape == (4, N, 14)
    assert got.sizes.tolist() == list(SIZES) and got.mask.sum(1).tolist() == list(SIZES)
    cast = np.zeros((4, N, N), dtype=np.float32)
    for b, C in enumerate(mats):
        cast[b, :C.shape[0], :C.shape[0]] = C.astype(np.float32)
    assert got.cost.dtype == torch.float32
    assert np.array_equal(got.cost.cpu().numpy().view(np.int32), cast.view(np.int32))
    assert got.u.dtype == got.v.dtype == torch.float32 and torch.isfinite(got.u).all()
    for b, n in enumerate(SIZES):
        assert (got.u[b, n:] == 0).all() and (got.v[b, n:] == 0).all()


def test_noisy_labels_with_a_seeded_generator(setup):
    torch, pipe, mats = setup
    clean = pipe.dual_training_batch(mats)
    g1 = torch.Generator(device="cuda:0").manual_seed(5)
    g2 = torch.Generator(device="cuda:0").manual_seed(5)
    noisy = pipe.dual_training_batch(mats, dual_noise_std=0.15, dual_noise_prob=1.0, generator=g1)
    want = pipe.training_batch(mats, dual_noise_std=0.15, dual_noise_prob=1.0, generator=g2)
    torch.cuda.synchronize()
    assert torch.equal(noisy.u, want.u) and torch.equal(noisy.v, want.v)
    assert not torch.equal(noisy.u, clean.u)
    for name in ("cost", "edge_feat", "row_feat", "col_feat", "mask", "sizes"):
        assert torch.equal(getattr(noisy, name), getattr(clean, name)), name


def test_one_training_step(setup):
    torch, pipe, mats = setup
    from gnn.losses import dual_warmstart_loss
    batch = pipe.dual_training_batch(mats)
    model = pipe.model
    model.fused_attention_training = True
    model.train()
    try:
        model.zero_grad(set_to_none=True)
        out = model(batch.edge_feat, batch.row_feat, batch.col_feat, sizes=batch.sizes)
        loss, metrics = dual_warmstart_loss(batch.cost, out["u"], out["v_hint"], batch.mask)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and (metrics["ret"] == 0).all() and torch.isfinite(metrics["v_reg"]).all()
        for name, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert any(float(p.grad.abs().max()) > 0 for p in model.col_out.parameters())  # v_hint was reached
        assert any(float(p.grad.abs().max()) > 0 for p in model.row_out.parameters())
    finally:
        model.eval()
        model.fused_attention_training = False
        model.zero_grad(set_to_none=True)
