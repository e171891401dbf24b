"""lapwarm_refine_backward on the MI355X through the C ABI, and the autograd path of OneGNN that uses it,
against the float64 references of tests/refine_backward_common.py and the float64 CPU model.

Tolerance everywhere (refine_backward_common.tolerance), per output or parameter: 4 x the max-abs error of
PyTorch-CPU float32 autograd of the reference op order on the same inputs, or 1e-6 * max(1, max|ref|) if that
is larger."""
import ctypes as ct

import numpy as np
import pytest

import dense_sweeps_common as dsc
import refine_backward_common as rbc
from test_gpu_dense_sweeps import gpu  # noqa: F401  (the module-scoped Device fixture)

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.0)
TAIL = 16  # one block of rows
INVALID = -2
NAMES = ("grad_u", "grad_w1", "grad_b1")


def _backward_call(gpu, top, u_pre, w1, b1, G, s, stream=None, ws=None):
    """One lapwarm_refine_backward call into sentinel-tailed outputs and a 0xFF workspace (NaN as fp64):
    (grad_u, grad_w1, grad_b1) as NumPy arrays; asserts that nothing behind them was written."""
    torch = gpu.torch
    rows, H = top.shape[0], w1.shape[0]
    gu = torch.full((rows + TAIL,), float(SENTINEL), dtype=torch.float32, device=gpu.dev)
    gw = torch.full((2 * H,), float(SENTINEL), dtype=torch.float32, device=gpu.dev)
    gb = torch.full((2 * H,), float(SENTINEL), dtype=torch.float32, device=gpu.dev)
    nbytes = gpu.lib.lapwarm_refine_backward_workspace_bytes(rows, H)
    assert nbytes > 0
    if ws is None:
        ws = gpu.poisoned((nbytes,), torch.uint8)
    assert ws.numel() >= nbytes
    td, ud, wd, bd, Gd = gpu.put(top), gpu.put(u_pre), gpu.put(w1), gpu.put(b1), gpu.put(G)
    sd = None if s is None else gpu.put(s)
    gpu.sync()
    handle = gpu.stream if stream is None else ct.c_void_p(stream.cuda_stream)
    rc = gpu.lib.lapwarm_refine_backward(td.data_ptr(), ud.data_ptr(), wd.data_ptr(), bd.data_ptr(), Gd.data_ptr(),
                                         None if sd is None else sd.data_ptr(), gu.data_ptr(), gw.data_ptr(),
                                         gb.data_ptr(), rows, H, ws.data_ptr(), nbytes, handle)
    gpu.sync()
    assert rc == 0
    gu, gw, gb = gu.cpu().numpy(), gw.cpu().numpy(), gb.cpu().numpy()
    assert (gu[rows:] == SENTINEL).all(), "grad_u written past `rows`"
    assert (gw[H:] == SENTINEL).all() and (gb[H:] == SENTINEL).all(), "grad_w1 / grad_b1 written past H"
    return gu[:rows], gw[:H], gb[:H]


# ----------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("H", [2, 3, 64, 192, 257])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33, 257])
def test_refine_backward(gpu, rows, H):
    """grad_u, grad_w1 and grad_b1 against the float64 closed form, on the moderate and the large inputs of
    test_refine_aggregate (full, +inf-padded, all-+inf, -inf / NaN, tied and widely spread rows), G, s ~ N(0, 1).

    Exact: a row without a finite value gives grad_u == 0; nothing is written behind grad_u (16 rows) or
    behind grad_w1 / grad_b1 (H entries); grad_wsum = NULL gives the bits of an all-zero grad_wsum.
    Tolerance: the module docstring's, separately per output and per input group, each pooled over the calls
    of one (rows, H).

    Not yet run on an MI355X: the test prints every figure before it asserts."""
    seen = set()
    for group, lst in rbc.input_groups(rows, H).items():
        err_gpu = dict.fromkeys(NAMES, 0.0)
        err_cpu = dict.fromkeys(NAMES, 0.0)
        big = dict.fromkeys(NAMES, 0.0)
        for n_call, ((top, u_pre, kinds), (w1, b1)) in enumerate(lst):
            import torch
            seen |= set(kinds)
            G, s = rbc.grad_seeds(rows, H, seed=n_call)
            ref = rbc.refine_backward_ref(top, u_pre, w1, b1, G, s)
            cpu = rbc.refine_autograd(top, u_pre, w1, b1, G, s, dtype=torch.float32)
            out = _backward_call(gpu, top, u_pre, w1, b1, G, s)
            dead = np.array([k == "masked" for k in kinds])
            assert (out[0][dead] == 0).all(), group
            for name, o, c, r in zip(NAMES, out, cpu, ref):
                assert np.isfinite(o).all(), (group, name)
                err_gpu[name] = max(err_gpu[name], float(np.abs(o.astype(np.float64) - r).max()))
                err_cpu[name] = max(err_cpu[name], float(np.abs(c.astype(np.float64) - r).max()))
                big[name] = max(big[name], float(np.abs(r).max()))
            if n_call == 0:
                zero = _backward_call(gpu, top, u_pre, w1, b1, G, np.zeros(rows, np.float32))
                null = _backward_call(gpu, top, u_pre, w1, b1, G, None)
                for a, b in zip(zero, null):
                    assert a.tobytes() == b.tobytes(), (group, "grad_wsum = NULL differs from zeros")
        for name in NAMES:
            tol = max(4.0 * err_cpu[name], 1e-6 * max(1.0, big[name]))
            print(f"refine backward rows={rows} H={H} {group} {name}: kernel {err_gpu[name]:.3e}, "
                  f"PyTorch-CPU float32 {err_cpu[name]:.3e}, tolerance {tol:.3e}, max|ref| {big[name]:.3e}")
        for name in NAMES:
            tol = max(4.0 * err_cpu[name], 1e-6 * max(1.0, big[name]))
            assert err_gpu[name] <= tol, (group, name, err_gpu[name], err_cpu[name])
    assert rows < 8 or seen == set(dsc.REFINE_KINDS)


def test_refine_backward_dead_rows_only(gpu):
    """Every row without a finite value: grad_u, grad_w1 and grad_b1 are exactly zero, NaN in G of such rows
    included (they add nothing)."""
    rows, H = 20, 5
    top = np.full((rows, dsc.K), np.inf, np.float32)
    u_pre = np.linspace(-1, 1, rows).astype(np.float32)
    w1, b1 = dsc.refine_weights(H)
    G, s = rbc.grad_seeds(rows, H)
    G[3, 2] = np.nan
    for out in _backward_call(gpu, top, u_pre, w1, b1, G, s):
        assert (out == 0).all()


def test_refine_backward_is_deterministic(gpu):
    """Two calls, and a call on a second stream that reuses the first call's workspace, give the same bits;
    rows = 40000 is above one tile per workgroup (2048 x 16 rows), so slabs are accumulated across tiles."""
    torch = gpu.torch
    for rows, H in ((257, 192), (40000, 24)):
        top, u_pre, _ = dsc.refine_inputs(rows, seed=9)
        w1, b1 = dsc.refine_weights(H, seed=9)
        G, s = rbc.grad_seeds(rows, H)
        nbytes = gpu.lib.lapwarm_refine_backward_workspace_bytes(rows, H)
        ws = gpu.poisoned((nbytes,), torch.uint8)
        first = _backward_call(gpu, top, u_pre, w1, b1, G, s, ws=ws)
        second = _backward_call(gpu, top, u_pre, w1, b1, G, s)
        side = torch.cuda.Stream(device=gpu.dev)
        third = _backward_call(gpu, top, u_pre, w1, b1, G, s, stream=side, ws=ws)
        for a, b, c in zip(first, second, third):
            assert a.tobytes() == b.tobytes() and a.tobytes() == c.tobytes()
        if rows > 2048 * 16:
            import torch as T
            ref = rbc.refine_backward_ref(top, u_pre, w1, b1, G, s)
            cpu = rbc.refine_autograd(top, u_pre, w1, b1, G, s, dtype=T.float32)
            for name, o, c, r in zip(NAMES, first, cpu, ref):
                err = float(np.abs(o.astype(np.float64) - r).max())
                assert err <= rbc.tolerance(float(np.abs(c.astype(np.float64) - r).max()), r), (name, err)


def test_refine_backward_argument_codes(gpu):
    """NULL required pointers, H = 0 and a short workspace return the invalid-argument code (-2) and launch
    nothing (the sentinels stay); rows = 0 returns 0."""
    torch = gpu.torch
    rows, H = 17, 3
    top, u_pre, _ = dsc.refine_inputs(rows)
    w1, b1 = dsc.refine_weights(H)
    G, s = rbc.grad_seeds(rows, H)
    t = [gpu.put(a) for a in (top, u_pre, w1, b1, G, s)]
    outs = [torch.full((k,), float(SENTINEL), dtype=torch.float32, device=gpu.dev) for k in (rows, H, H)]
    lib = gpu.lib
    nbytes = lib.lapwarm_refine_backward_workspace_bytes(rows, H)
    assert nbytes > 0 and lib.lapwarm_refine_backward_workspace_bytes(0, H) == 0
    ws = gpu.poisoned((nbytes,), torch.uint8)
    good = [x.data_ptr() for x in t] + [x.data_ptr() for x in outs]

    def call(ptrs, rows_, H_, ws_ptr, ws_bytes):
        rc = lib.lapwarm_refine_backward(*ptrs, rows_, H_, ws_ptr, ws_bytes, gpu.stream)
        gpu.sync()
        return rc

    for k in (0, 1, 2, 3, 4, 6, 7, 8):  # every pointer but grad_wsum
        ptrs = list(good)
        ptrs[k] = None
        assert call(ptrs, rows, H, ws.data_ptr(), nbytes) == INVALID, k
    assert call(good, rows, H, None, nbytes) == INVALID
    assert call(good, rows, 0, ws.data_ptr(), nbytes) == INVALID
    assert call(good, rows, -1, ws.data_ptr(), nbytes) == INVALID
    assert call(good, -1, H, ws.data_ptr(), nbytes) == INVALID
    assert call(good, rows, H, ws.data_ptr(), nbytes - 1) == INVALID
    assert call(good, 0, H, ws.data_ptr(), nbytes) == 0
    assert call(good, 0, H, None, 0) == 0
    for o in outs:
        assert (o == float(SENTINEL)).all()
    assert call(good, rows, H, ws.data_ptr(), nbytes) == 0
    assert all((o != float(SENTINEL)).all() for o in outs)


# ------------------------------------------------------------------------------------------------ the model
def _case(gpu, n, masked):
    """Row features and top-16 values of B = 2 random instances on the device, a mask, and output weights."""
    torch = gpu.torch
    from gnn.features import row_features_device
    B = 2
    C32 = np.random.RandomState(n).uniform(0.0, 1.0, (B, n, n)).astype(np.float32)
    feat, topk = row_features_device(gpu.put(C32.astype(np.float64)))
    mask = torch.ones((B, n), dtype=torch.bool)
    if masked:
        mask[0, 0] = mask[0, 7] = mask[1, n - 1] = False
    weight = torch.from_numpy(np.random.RandomState(n + 1).normal(0.0, 1.0, (B, n)).astype(np.float32))
    return feat, topk, mask, weight


def _grads(model, feat, topk, mask, weight):
    model.zero_grad(set_to_none=True)
    u = model(feat, topk_values=topk, mask=mask)["u"]
    (u * weight).sum().backward()
    return u.detach(), {k: p.grad for k, p in model.named_parameters()}


def _cpu_model(sd, dtype, train):
    from gnn import OneGNN
    model = OneGNN(21, hidden=64, layers=2, dropout=0.0).to(dtype)
    model.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    return model.train() if train else model.eval()


def _check_against_cpu(gpu, model, sd, case, train):
    """u and every parameter gradient of the device model against the float64 CPU model (reference op order),
    each within the module docstring's tolerance, with the float32 CPU model as the yardstick."""
    torch = gpu.torch
    feat, topk, mask, weight = case
    u, grads = _grads(model, feat, topk, mask.to(gpu.dev), weight.to(gpu.dev))
    for name in ("pre_out.weight", "edge_mlp.0.weight", "edge_mlp.0.bias"):
        assert grads[name] is not None, f"{name} received no gradient through the fused refinement"
    fc, tc = feat.cpu(), topk.cpu()
    u64, g64 = _grads(_cpu_model(sd, torch.float64, train), fc.double(), tc.double(), mask, weight.double())
    u32, g32 = _grads(_cpu_model(sd, torch.float32, train), fc.float(), tc.float(), mask, weight)
    worst = 0.0
    for name, ref in [("u", u64)] + sorted(g64.items()):
        got = u if name == "u" else grads[name]
        cpu = u32 if name == "u" else g32[name]
        assert got is not None and ref is not None, name
        ref = ref.numpy()
        err = float(np.abs(got.cpu().double().numpy() - ref).max())
        tol = rbc.tolerance(float(np.abs(cpu.double().numpy() - ref).max()), ref)
        print(f"{name}: device {err:.3e}, tolerance {tol:.3e}, max|ref| {np.abs(ref).max():.3e}")
        worst = max(worst, err / tol)
        assert err <= tol, (name, err, tol)
    assert (u[~mask.to(gpu.dev)] == 0).all()
    return worst


def _device_model(gpu, dropout=0.1):
    torch = gpu.torch
    from gnn import OneGNN
    torch.manual_seed(5)
    model = OneGNN(21, hidden=64, layers=2, dropout=dropout)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model.to(gpu.dev), sd


@pytest.mark.parametrize("n,masked", [(12, False), (40, True)], ids=["n12_padded", "n40_masked"])
def test_eval_mode_gradient_reaches_u_pre_and_the_first_edge_layer(gpu, n, masked):
    """OneGNN(21, hidden=64, layers=2).eval() on the device with topk_values= (n = 12: four +inf per row;
    n = 40 with masked rows): after (u * weight).sum().backward(), pre_out.weight, edge_mlp[0].weight and
    edge_mlp[0].bias have gradients, and every parameter gradient agrees with the float64 CPU model, which
    takes the reference op order.  Without the backward kernel the first assertion fails: autograd saw no edge
    from the aggregate back to u_pre and the first edge-MLP layer.

    Not yet run on an MI355X: the test prints every figure before it asserts."""
    model, sd = _device_model(gpu)
    worst = _check_against_cpu(gpu, model.eval(), sd, _case(gpu, n, masked), train=False)
    print(f"n={n}: largest error / tolerance {worst:.2f}")


def _forward_in_reference_order(model, feat, topk, mask):
    """OneGNN.forward with _refine_reference_order called directly."""
    h = model.input_proj(feat)
    for block in model.blocks:
        h = block(h)
    u_pre = model.pre_out(h).squeeze(-1)
    h = h + model._refine_reference_order(h, topk[..., :16], u_pre, mask.unsqueeze(-1))
    u = model.row_out(h).squeeze(-1)
    u = u - u.mean(dim=-1, keepdim=True)
    return u.masked_fill(~mask, 0.0)


def test_training_mode_default_is_the_reference_order(gpu):
    """fused_refine_training defaults to False: model.train() (dropout = 0) gives the bits of the forward
    with _refine_reference_order called directly, and never enters the fused path."""
    torch = gpu.torch
    model, _ = _device_model(gpu, dropout=0.0)
    model.train()
    assert model.fused_refine_training is False
    feat, topk, mask, _ = _case(gpu, 40, True)
    mask = mask.to(gpu.dev)
    calls = []
    fused = model._refine_fused
    model._refine_fused = lambda *a: calls.append(1) or fused(*a)
    u = model(feat, topk_values=topk, mask=mask)["u"]
    assert not calls
    assert torch.equal(u, _forward_in_reference_order(model, feat, topk, mask))
    model.fused_refine_training = True
    model(feat, topk_values=topk, mask=mask)
    assert calls == [1]


@pytest.mark.parametrize("n,masked", [(12, False), (40, True)], ids=["n12_padded", "n40_masked"])
def test_fused_refine_training_matches_the_cpu_model(gpu, n, masked):
    """fused_refine_training = True, dropout = 0: outputs and all parameter gradients of model.train() on
    the device agree with the float64 CPU model in training mode.

    Not yet run on an MI355X: the test prints every figure before it asserts."""
    model, sd = _device_model(gpu, dropout=0.0)
    model.train()
    model.fused_refine_training = True
    worst = _check_against_cpu(gpu, model, sd, _case(gpu, n, masked), train=True)
    print(f"n={n}: largest error / tolerance {worst:.2f}")


def test_eval_forward_does_not_depend_on_the_switch(gpu):
    """Eval mode under no_grad and under inference_mode: the same bits with fused_refine_training either
    way, and the bits of the aggregation entry point the forward has always used."""
    torch = gpu.torch
    model, _ = _device_model(gpu)
    model.eval()
    feat, topk, mask, _ = _case(gpu, 40, True)
    mask = mask.to(gpu.dev)
    with torch.no_grad():
        u0 = model(feat, topk_values=topk, mask=mask)["u"]
        model.fused_refine_training = True
        u1 = model(feat, topk_values=topk, mask=mask)["u"]
    with torch.inference_mode():
        u2 = model(feat, topk_values=topk, mask=mask)["u"]
    assert torch.equal(u0, u1) and torch.equal(u0, u2)
    assert not u0.requires_grad


def test_training_step_with_dropout_runs_and_is_finite(gpu):
    """fused_refine_training with dropout on: one step through warm-start loss and backward; every parameter
    gets a finite gradient (dropout makes the values random, so nothing more is compared)."""
    torch = gpu.torch
    from gnn.losses import warmstart_loss
    model, _ = _device_model(gpu, dropout=0.1)
    model.train()
    model.fused_refine_training = True
    B, n = 2, 40
    C32 = np.random.RandomState(n).uniform(0.0, 1.0, (B, n, n)).astype(np.float32)
    feat, topk, mask, _ = _case(gpu, n, False)
    cost = gpu.put(C32)
    u = model(feat, topk_values=topk, mask=mask.to(gpu.dev))["u"]
    loss, _ = warmstart_loss(cost, u, cost.min(dim=2).values, mask.to(gpu.dev))
    loss.backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
