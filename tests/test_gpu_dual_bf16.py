"""The bf16 edge MLP of DualGNN on the MI355X (fused_edge_precision = "bf16") against the torch restatement of its
arithmetic contract (dual_bf16_common), never against the kernels themselves.

Forward, per case: (a) every score within the flip bound B = 2^-7 max|G| max|h2| of the fp64 restatement (two worst-case
flips of a rounded h2; B from the restatement); (b) at most 1 % of the scores further than 1e-5 from it.
Backward: per gradient tensor max|difference| / max|reference| against fp64 autograd through the straight-through
restatement, bounded by 4 x the figure recorded in profiles/dual_gnn_bf16.md (GRAD_RECORDED below) and never above
2^-6 (four stacked bf16 half-ulps): where 4 x the recorded figure is larger (b1 at heads 8, b1 and b2 with sizes:
1.64e-2, 1.73e-2, 1.83e-2) the bound is 2^-6 = 1.5625e-2, the tighter of the two."""
import numpy as np
import pytest
import torch

import dual_bf16_common as bc
import dual_dropout_common as ddc
import test_gpu_dual_backward as tgb
from host_common import device_lib as lib  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = tgb.SENTINEL
_stream, _ptr = tgb._stream, tgb._ptr
NAMES = ("W1", "b1", "W2", "b2", "G")
P, SEED_DROP = 0.1, 4242

# max|difference| / max|reference| per gradient, measured on the MI355X (profiles/dual_gnn_bf16.md)
GRAD_RECORDED = {
    "B=1 N=5 heads=4": {"W1": 2.152e-03, "b1": 2.471e-03, "W2": 2.944e-03, "b2": 2.047e-03, "G": 1.298e-03},
    "B=2 N=12 heads=1": {"W1": 2.954e-03, "b1": 1.919e-03, "W2": 3.804e-03, "b2": 2.838e-03, "G": 1.667e-03},
    "B=2 N=12 heads=8": {"W1": 3.746e-03, "b1": 4.099e-03, "W2": 2.608e-03, "b2": 3.377e-03, "G": 1.271e-03},
    "B=1 N=176 heads=4": {"W1": 3.540e-03, "b1": 2.902e-03, "W2": 3.156e-03, "b2": 2.816e-03, "G": 1.320e-03},
    "sizes": {"W1": 3.585e-03, "b1": 4.333e-03, "W2": 2.642e-03, "b2": 4.576e-03, "G": 1.486e-03},
    "dropout": {"W1": 2.836e-03, "b1": 2.639e-03, "W2": 2.463e-03, "b2": 2.046e-03, "G": 1.391e-03},
}


def _forward(lib, d, sizes, B, N, heads, seed=0, p=0.0, fill=SENTINEL):
    scores = torch.full((B, 2 * heads, N, N), fill, device=DEV)
    rc = lib.lapwarm_dual_edge_scores_bf16(*[t.data_ptr() for t in d], scores.data_ptr(), _ptr(sizes), B, N, heads,
                                           seed, p, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return scores.cpu()


def _backward(lib, d, dS, sizes, B, N, heads, seed=0, p=0.0):
    nbytes = int(lib.lapwarm_dual_backward_workspace_bytes(B, N, heads))
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    out = [torch.full_like(t, SENTINEL) for t in d[1:]]
    rc = lib.lapwarm_dual_edge_scores_backward_bf16(*[t.data_ptr() for t in d], dS.data_ptr(), _ptr(sizes),
                                                    *[t.data_ptr() for t in out], B, N, heads, ws.data_ptr(), nbytes,
                                                    seed, p, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return dict(zip(NAMES, (t.cpu() for t in out)))


def _check_forward(label, got, args, mask0=None, inside=None):
    want, h2_max, g_max = bc.edge_scores(*args, mask0, dtype=torch.float64, parts=True)
    share, worst = bc.share_and_max(got, want, inside)
    bound = bc.flip_bound(h2_max, g_max)
    print(f"BF16-FWD {label}: share {share:.5f} max {worst:.3e} flip bound {bound:.3e}")
    assert worst <= bound, label
    assert share <= bc.SHARE_CAP, label


def _check_gradients(label, got, want):
    errs = {n: float((got[n].double() - want[n]).abs().max() / want[n].abs().max()) for n in NAMES}
    print(f"BF16-BWD {label}: " + ", ".join(f'"{n}": {errs[n]:.3e}' for n in NAMES))
    for n in NAMES:
        assert torch.isfinite(got[n]).all(), (label, n)
        bound = min(4.0 * GRAD_RECORDED[label][n], bc.GRAD_CAP)  # three of the thirty would pass the cap: it holds
        assert errs[n] <= bound, (label, n, errs[n], bound)


def _dS(B, N, heads, seed=3):
    return torch.randn((B, 2 * heads, N, N), generator=torch.Generator().manual_seed(seed + N + heads))


# ---- forward ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N,heads", bc.FORWARD_SHAPES)
def test_scores_meet_the_flip_bound_and_the_share_cap(lib, B, N, heads):
    args = bc.inputs(B, N, heads)
    d = [t.to(DEV) for t in args]
    got = _forward(lib, d, None, B, N, heads)
    _check_forward(f"B={B} N={N} heads={heads}", got, args)
    assert torch.equal(got, _forward(lib, d, None, B, N, heads))  # equal inputs, equal bits


def test_scores_with_sizes_are_the_uniform_bits_on_the_prefixes_and_leave_the_rest(lib):
    sizes, N, heads = bc.RAGGED_SIZES, bc.RAGGED_N, 4
    B = len(sizes)
    args = bc.inputs(B, N, heads)
    d = [t.to(DEV) for t in args]
    uniform = _forward(lib, d, None, B, N, heads)
    ragged = _forward(lib, d, torch.tensor(sizes, dtype=torch.int32, device=DEV), B, N, heads)
    inside = bc.prefix_mask(sizes, N)[:, None].expand(B, 2 * heads, N, N)
    assert torch.equal(ragged[inside], uniform[inside])
    assert bool((ragged[~inside] == SENTINEL).all())
    _check_forward("sizes", ragged, args, inside=inside)


def test_fp32_entry_keeps_its_bits_and_bf16_differs(lib):
    B, N, heads = 2, 12, 4
    args = bc.inputs(B, N, heads)
    d = [t.to(DEV) for t in args]
    from gnn.dual_gnn import _EdgeScores
    with torch.no_grad():
        fp32 = _EdgeScores.apply(*d, None).cpu()                       # the switch at "fp32": the default argument
        bf16 = _EdgeScores.apply(*d, None, 0, 0.0, "bf16").cpu()
    plain = torch.empty((B, 2 * heads, N, N), device=DEV)
    assert lib.lapwarm_dual_edge_scores(*[t.data_ptr() for t in d], plain.data_ptr(), B, N, heads, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(fp32.reshape(plain.shape), plain.cpu())
    assert torch.equal(bf16.reshape(plain.shape), _forward(lib, d, None, B, N, heads))
    assert not torch.equal(fp32, bf16)


# ---- backward --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N,heads", bc.BACKWARD_SHAPES)
def test_gradients_against_fp64_autograd_through_the_restatement(lib, B, N, heads):
    args = bc.inputs(B, N, heads)
    dS = _dS(B, N, heads)
    d = [t.to(DEV) for t in args]
    got = _backward(lib, d, dS.to(DEV), None, B, N, heads)
    _check_gradients(f"B={B} N={N} heads={heads}", got, bc.edge_gradients(*args, dS))
    again = _backward(lib, d, dS.to(DEV), None, B, N, heads)
    assert all(torch.equal(got[n], again[n]) for n in NAMES)


def test_gradients_with_sizes(lib):
    sizes, N, heads = bc.RAGGED_SIZES, bc.RAGGED_N, 4
    B = len(sizes)
    args = bc.inputs(B, N, heads)
    inside = bc.prefix_mask(sizes, N)[:, None].expand(B, 2 * heads, N, N)
    dS = _dS(B, N, heads)
    d = [t.to(DEV) for t in args]
    # outside the prefixes the kernel must not read dS: NaN there on the device, 0 in the reference
    got = _backward(lib, d, torch.where(inside, dS, torch.tensor(float("nan"))).to(DEV),
                    torch.tensor(sizes, dtype=torch.int32, device=DEV), B, N, heads)
    _check_gradients("sizes", got, bc.edge_gradients(*args, torch.where(inside, dS, torch.tensor(0.0))))


def test_the_workspace_request_is_unchanged(lib):
    from gnn.dual_gnn import _backward_workspace
    for B, N, heads in bc.BACKWARD_SHAPES:
        ws = _backward_workspace(lib, B, N, heads, torch.device(DEV))
        assert ws.numel() == int(lib.lapwarm_dual_backward_workspace_bytes(B, N, heads))
    args = bc.inputs(1, 5, 4)
    d = [t.to(DEV) for t in args]
    out = [torch.empty_like(t) for t in d[1:]]
    dS = _dS(1, 5, 4).to(DEV)
    nbytes = int(lib.lapwarm_dual_backward_workspace_bytes(1, 5, 4))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    short = lib.lapwarm_dual_edge_scores_backward_bf16(*[t.data_ptr() for t in d], dS.data_ptr(), None,
                                                       *[t.data_ptr() for t in out], 1, 5, 4, ws.data_ptr(), nbytes - 1,
                                                       0, 0.0, _stream())
    assert short == -1


# ---- dropout ---------------------------------------------------------------------------------------------------

def test_dropout_forward_and_backward_with_the_mask_of_the_fp32_path(lib):
    B, N, heads = 2, 12, 4
    args = bc.inputs(B, N, heads)
    d = [t.to(DEV) for t in args]
    keep = torch.empty((B * N * N * bc.EDGE_HIDDEN,), dtype=torch.uint8, device=DEV)
    assert lib.lapwarm_dual_dropout_keep(SEED_DROP, 0, 0, keep.numel(), P, keep.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    mask0 = keep.cpu().reshape(B, N, N, bc.EDGE_HIDDEN).float() * float(np.float32(1.0 / (1.0 - P)))
    got = _forward(lib, d, None, B, N, heads, SEED_DROP, P)
    _check_forward("dropout", got, args, mask0)
    assert torch.equal(got, _forward(lib, d, None, B, N, heads, SEED_DROP, P))
    assert not torch.equal(got, _forward(lib, d, None, B, N, heads))
    dS = _dS(B, N, heads)
    grads = _backward(lib, d, dS.to(DEV), None, B, N, heads, SEED_DROP, P)
    _check_gradients("dropout", grads, bc.edge_gradients(*args, dS, mask0))
    # the kept set is that of the fp32 path: its scores match the fp32 restatement with this very mask
    fp32 = torch.empty((B, 2 * heads, N, N), device=DEV)
    assert lib.lapwarm_dual_edge_scores_dropout(*[t.data_ptr() for t in d], fp32.data_ptr(), None, B, N, heads,
                                                SEED_DROP, P, _stream()) == 0
    torch.cuda.synchronize()
    want = ddc.edge_scores_torch(*[t.double() for t in args], mask0).reshape(fp32.shape)
    assert float((fp32.cpu().double() - want).abs().max()) <= bc.ONEGNN_ABS
    assert torch.equal(mask0 != 0, ddc.edge_mask(SEED_DROP, P, B, N) != 0)


# ---- the model -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model_case():
    from gnn.dual_gnn import DualGNN
    from solvers.generators import mixed_batch
    C_host, _ = mixed_batch(2, 48, families=("uniform", "clustered"), seed=11)
    torch.manual_seed(0)
    model = DualGNN(hidden_dim=128, layers=2, heads=4).to(DEV).eval()
    return model, C_host


def test_model_under_bf16_is_finite_and_ignores_autocast(lib, model_case):
    model, C_host = model_case
    from gnn.pipeline import DualWarmStartPipeline
    pipe = DualWarmStartPipeline(model, DEV)
    C = torch.from_numpy(C_host).to(DEV)
    model.fused_edge_precision = "fp32"
    u32 = pipe.solve_batch(C)["u"].clone()
    model.fused_edge_precision = "bf16"
    try:
        u16 = pipe.solve_batch(C)["u"].clone()
        with torch.autocast("cuda"):
            u16_auto = pipe.solve_batch(C)["u"].clone()
    finally:
        model.fused_edge_precision = "fp32"
    torch.cuda.synchronize()
    print(f"BF16-MODEL max|u_bf16 - u_fp32| = {float((u16 - u32).abs().max()):.3e}, max|u| = {float(u32.abs().max()):.3e}")
    assert torch.isfinite(u16).all()
    assert torch.equal(u16, u16_auto)
    assert not torch.equal(u16, u32)


def test_pipeline_with_the_bf16_model_returns_optimal_permutations(lib, model_case):
    model, C_host = model_case
    from gnn.pipeline import DualWarmStartPipeline
    pipe = DualWarmStartPipeline(model, DEV)
    model.fused_edge_precision = "bf16"
    try:
        out = pipe.solve_batch(torch.from_numpy(C_host).to(DEV))
    finally:
        model.fused_edge_precision = "fp32"
    torch.cuda.synchronize()
    x = out["x"].cpu().numpy()
    x_cold = pipe.lapjv_batch(torch.from_numpy(C_host).to(DEV))[0].cpu().numpy()
    n = C_host.shape[1]
    for b in range(C_host.shape[0]):
        assert np.array_equal(np.sort(x[b]), np.arange(n)), b
        cost, want = C_host[b][np.arange(n), x[b]].sum(), C_host[b][np.arange(n), x_cold[b]].sum()
        # two optimal assignments of one fp64 matrix with entries <= 100: their sums differ by rounding only
        assert abs(cost - want) <= 1e-9 * max(1.0, abs(want)), (b, cost, want)


def test_one_training_step_gives_every_parameter_a_finite_gradient(lib, model_case):
    """forward, dual_warmstart_loss, backward on a labelled batch of the pipeline (its matching from the seeded solve)"""
    model, C_host = model_case
    from gnn.losses import dual_warmstart_loss
    from gnn.pipeline import DualWarmStartPipeline
    pipe = DualWarmStartPipeline(model, DEV)
    model.fused_edge_precision = "bf16"
    model.fused_attention_training = True
    model.train()
    try:
        batch = pipe.dual_training_batch([np.ascontiguousarray(C) for C in C_host])
        model.zero_grad(set_to_none=True)
        out = model(batch.edge_feat, batch.row_feat, batch.col_feat, sizes=batch.sizes)
        loss, metrics = dual_warmstart_loss(batch.cost, out["u"], out["v_hint"], batch.mask)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and (metrics["ret"] == 0).all()
        for name, prm in model.named_parameters():
            assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
        lin = model.layers[0].edge_mlp[3]
        assert float(lin.weight.grad.abs().max()) > 0  # the bf16 edge backward was reached
    finally:
        model.eval()
        model.fused_attention_training = False
        model.fused_edge_precision = "fp32"
        model.zero_grad(set_to_none=True)
