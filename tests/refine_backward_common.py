"""References for the backward of the refinement aggregation (csrc/onegnn_refine.hip,
lapwarm_refine_backward) -- TEST INFRASTRUCTURE, no GPU needed.

`refine_backward_ref` restates the closed form of include/lapwarm_hip.h in float64; `refine_autograd` is
torch autograd of the same ops, in the same order, as OneGNN._refine_reference_order before its second linear
layer, in a dtype of the caller's choice: float64 to check the closed form, float32 as the yardstick of what
float32 arithmetic costs.  Inputs come from dense_sweeps_common.refine_inputs / refine_weights."""
import numpy as np

import dense_sweeps_common as dsc

K = dsc.K


def refine_backward_ref(topk16, u_pre, w1, b1, G, s=None):
    """float64 restatement of lapwarm_refine_backward: (grad_u (rows,), grad_w1 (H,), grad_b1 (H,)).
    val = float32(topk) - float32(u_pre) is formed in float32, as dsc.refine_aggregate_ref and the kernels form
    it; everything after it is float64.  G (rows, H) = dL/dagg, s (rows,) = dL/dwsum or None for zero."""
    import torch
    G = np.asarray(G, np.float64)
    rows = G.shape[0]
    s = np.zeros(rows) if s is None else np.asarray(s, np.float64)
    w1 = np.asarray(w1, np.float64)
    b1 = np.asarray(b1, np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        val = (np.asarray(topk16, np.float32) - np.asarray(u_pre, np.float32)[:, None]).astype(np.float64)
        ok = np.isfinite(val)
        val0 = np.where(ok, val, 0.0)
        mn = np.where(ok, val, np.inf).min(axis=1, keepdims=True)
        e = np.where(ok, np.exp(-(val0 - np.where(np.isfinite(mn), mn, 0.0))), 0.0)
        tot = e.sum(axis=1, keepdims=True)
        w = np.where(tot > 0, e / np.where(tot > 0, tot, 1.0), 0.0)
        x = w1[None, None, :] * val0[:, :, None] + b1[None, None, :]
        cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(x) * 0.70710678118654752440).numpy())
        pdf = np.exp(-0.5 * x * x) * 0.39894228040143267794
        gelu = x * cdf
        dgelu = cdf + x * pdf
        Q = np.einsum("rh,rkh->rk", G, gelu) + s[:, None]
        D = np.einsum("rh,h,rkh->rk", G, w1, dgelu)
        dval = np.where(ok, w * D - w * (Q - (w * Q).sum(axis=1, keepdims=True)), 0.0)
        t = G[:, None, :] * w[:, :, None] * dgelu
        return -dval.sum(axis=1), (t * val0[:, :, None]).sum(axis=(0, 1)), t.sum(axis=(0, 1))


def refine_autograd(topk16, u_pre, w1, b1, G, s=None, dtype=None):
    """torch (CPU) autograd of  sum(G * agg) + sum(s * wsum)  with agg, wsum computed op for op as
    OneGNN._refine_reference_order does before its second linear layer (dsc.refine_aggregate_f32 with a graph),
    everything in `dtype`: (grad_u, grad_w1, grad_b1) as NumPy arrays of that dtype."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float32
    base = torch.from_numpy(np.asarray(topk16, np.float32)).to(dtype)
    up = torch.from_numpy(np.asarray(u_pre, np.float32)).to(dtype).requires_grad_()
    wt = torch.from_numpy(np.asarray(w1, np.float32)).to(dtype).view(-1, 1).requires_grad_()
    bt = torch.from_numpy(np.asarray(b1, np.float32)).to(dtype).requires_grad_()
    values = base - up.unsqueeze(-1)
    valid = torch.isfinite(values)
    neg = torch.where(valid, -values, torch.full_like(values, -float("inf")))
    w = torch.softmax(neg, dim=-1)
    w = torch.where(valid, w, torch.zeros_like(w))
    e_in = torch.where(valid, values, torch.zeros_like(values)).unsqueeze(-1)
    e = F.gelu(F.linear(e_in, wt, bt))
    agg = (w.unsqueeze(-1) * e).sum(dim=-2)
    loss = (torch.from_numpy(np.asarray(G)).to(dtype) * agg).sum()
    if s is not None:
        loss = loss + (torch.from_numpy(np.asarray(s)).to(dtype) * w.sum(dim=-1)).sum()
    loss.backward()
    return up.grad.numpy(), wt.grad.view(-1).numpy(), bt.grad.numpy()


def grad_seeds(rows, H, seed=0):
    """G ~ N(0, 1) (rows, H) and s ~ N(0, 1) (rows,), float32."""
    rs = np.random.RandomState([seed, rows, H, 82])
    return rs.normal(0.0, 1.0, (rows, H)).astype(np.float32), rs.normal(0.0, 1.0, rows).astype(np.float32)


def input_groups(rows, H):
    """The calls of test_refine_aggregate for one (rows, H): {"moderate": [...], "large": [...]}, each entry
    ((topk16, u_pre, kinds), (w1, b1)).  moderate: u_pre, w1, b1 ~ N(0, 1); large: u_pre = +-1e3, and
    w1, b1 x 50 for the GELU tails."""
    shifts = range(len(dsc.REFINE_KINDS)) if rows < len(dsc.REFINE_KINDS) else (0, 3)
    calls = {"moderate": [], "large": []}
    for sh in shifts:
        calls["moderate"].append((dsc.refine_inputs(rows, seed=H, shift=sh), dsc.refine_weights(H, seed=sh)))
    for sh in shifts:
        off = 1e3 if sh % 2 == 0 else -1e3
        calls["large"].append((dsc.refine_inputs(rows, seed=H + 1, shift=sh, u_offset=off),
                               dsc.refine_weights(H, seed=sh)))
        calls["large"].append((dsc.refine_inputs(rows, seed=H + 2, shift=sh),
                               dsc.refine_weights(H, seed=sh, scale=50.0)))
    return calls


def tolerance(err_f32, ref):
    """The bound of the forward's test, per output: 4 x the max-abs error of PyTorch-CPU float32 on the same
    inputs (another summation order, other expf / erff, all float32), or 1e-6 * max(1, max|ref|) if larger."""
    return max(4.0 * err_f32, 1e-6 * max(1.0, float(np.abs(ref).max())))
