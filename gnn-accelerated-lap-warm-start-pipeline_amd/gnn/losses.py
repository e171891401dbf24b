"""The training losses on the MI355X as HIP kernels (csrc/train_loss.hip), forward and backward: OneGNN's,
`compute_loss` of the reference's gnn/train_one_gnn.py:180-226 with its greedy primal bound (`greedy_primal_upper`,
:137-177; `greedy_primal_upper_np` of eval.py), as `warmstart_loss`; and DualGNN's, `compute_loss` of
gnn/train.py:267-308 (the same body in gnn/train_progressive.py:226-281), as `dual_warmstart_loss`.

Per instance with n_b valid rows and columns:

    v_j          = min_i (C_ij - u_i)                        (a_j: the row attaining it)
    dual_lower   = sum_i u_i + sum_j v_j
    feas         = sum_ij relu((u_i + v_j) - C_ij) / n_b^2
    u_reg        = sum_i (u_i - u_target_i)^2 / n_b
    primal_upper = cost of the greedy assignment on (C_ij - u_i) - v_j   (a constant for autograd)
    loss         = w0 mean_b(primal_upper - dual_lower) + w1 mean_b(feas) + w2 mean_b(u_reg)

DualGNN's loss has another third term, on the model's second output v_hint:

    v_reg        = sum_j (v_hint_j - v_j)^2 / n_b
    loss         = w0 mean_b(primal_upper - dual_lower) + w1 mean_b(feas) + w2 mean_b(v_reg)

It sends 2 (v_hint_j - v_j) / n_b into v_hint_j and, because v_j = C_{a_j j} - u_{a_j}, the sum of those over the
columns with a_j = i into u_i: an fp64 sum in ascending j without floating-point atomics, so equal inputs give
equal bits.

The float32 terms are the reference's; every sum is accumulated in fp64 and rounded to float32 once, so the
values differ from the reference's float32 sums by its summation error, not by more.

Ties.  Every row that attains a column minimum has a reduced cost of exactly 0 there, so the reference's two
`np.argsort` calls always sort ties, with numpy's default unstable sort: its `primal_upper` depends on the
numpy build.  Here ties go to the lowest index, as `kind="stable"` would order them: in the greedy's row
order, in the column a row takes, and in a_j.  The gradient does not depend on the greedy.

`mask` must be a prefix mask (`collate`, :72-91: instance b occupies rows and columns 0..n_b-1 of the padded
matrix); only its row sums are used and the prefix property is not checked.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from lap import _hip
from ._call import hip_call

__all__ = ["warmstart_loss", "greedy_primal_upper_batch"]

DEFAULT_WEIGHTS = (1.0, 1.0, 0.1)  # primal gap, feasibility, u regulariser (train_one_gnn.py:215-219)


def _check_args(cost, u_pred, u_target, mask, v_hint=None):
    """Argument errors, raised before any device work: types and dtypes, then shapes, then devices.  v_hint: the
    second prediction of the DualGNN loss, checked like u_pred, behind it."""
    half = (torch.float16, torch.bfloat16, torch.float32)
    args = [("cost", cost, (torch.float32,)), ("u_pred", u_pred, half)]
    if v_hint is not None:
        args.append(("v_hint", v_hint, half))
    if u_target is not None:
        args.append(("u_target", u_target, (torch.float32,)))
    if mask is not None:
        args.append(("mask", mask, (torch.bool,)))
    for name, t, dtypes in args:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"Argument '{name}' must be a torch.Tensor, not {type(t).__name__}")
        if t.dtype not in dtypes:
            raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")
    if cost.ndim != 3 or cost.shape[1] != cost.shape[2]:
        raise ValueError(f"cost must be (B, n, n), not {tuple(cost.shape)}")
    B, n = cost.shape[0], cost.shape[1]
    if B < 1 or n < 1:
        raise ValueError(f"cost must hold at least one instance of at least one row, not {tuple(cost.shape)}")
    if B > 65535:
        raise ValueError(f"at most 65535 instances per call, not {B}")
    if n > 16384:
        raise ValueError(f"n exceeds the 16384 limit of this build: {n}")
    for name, t, _ in args[1:]:
        if tuple(t.shape) != (B, n):
            raise ValueError(f"{name} must be ({B}, {n}) like cost, not {tuple(t.shape)}")
    if not cost.is_cuda:
        raise ValueError("cost must be on the GPU: the loss has no CPU path")
    for name, t, _ in args[1:]:
        if t.device != cost.device:
            raise ValueError(f"{name} must be on {cost.device} like cost, not {t.device}")
    return B, n


_WEIGHTS_ON_DEVICE = {}  # (device, the three numbers) -> float32 tensor: one upload per distinct triple


def _device_weights(weights, device):
    """The weights as a float32 tensor on `device`.  A tensor is taken as it is (it must be there already); a
    tuple of numbers is uploaded the first time it is seen on that device and kept, so that a training loop
    copies nothing from the host per step."""
    if isinstance(weights, torch.Tensor):
        if weights.device != device:
            raise ValueError(f"a weights tensor must be on {device} like cost, not {weights.device}")
        return weights.detach().contiguous()
    key = (device, tuple(float(x) for x in weights))
    if key not in _WEIGHTS_ON_DEVICE:
        _WEIGHTS_ON_DEVICE[key] = torch.tensor(key[1], dtype=torch.float32, device=device)
    return _WEIGHTS_ON_DEVICE[key]


def _forward(cost, u, u_target, sizes):
    """lapwarm_train_loss_forward on the current stream: v_proj, argmin_row, assign, terms, ret, workspace."""
    lib = _hip.require_device()
    B, n = cost.shape[0], cost.shape[1]
    dev = cost.device
    v_proj = torch.empty((B, n), dtype=torch.float32, device=dev)
    argmin_row = torch.empty((B, n), dtype=torch.int32, device=dev)
    assign = torch.empty((B, n), dtype=torch.int32, device=dev)
    terms = torch.empty((B, 4), dtype=torch.float32, device=dev)
    ret = torch.empty((B,), dtype=torch.int32, device=dev)
    nbytes = int(lib.lapwarm_train_loss_workspace_bytes(B, n))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    hip_call("lapwarm_train_loss_forward", "train_loss_forward", dev, cost, B, n, sizes, u, u_target, v_proj,
             argmin_row, assign, terms, ret, ws, nbytes)
    return v_proj, argmin_row, assign, terms, ret, ws


class _WarmstartLoss(torch.autograd.Function):
    """loss = w0 mean(primal_upper - dual_lower) + w1 mean(feas) + w2 mean(u_reg); differentiable in u_pred.
    The backward is one call of lapwarm_train_loss_backward with grad_scale = 1 / B and the weights
    multiplied by the incoming gradient on the device: nothing is added to what the kernel returns."""

    @staticmethod
    def forward(ctx, u_pred, cost, u_target, sizes, weights):
        u = u_pred.detach().to(torch.float32).contiguous()
        v_proj, argmin_row, assign, terms, ret, ws = _forward(cost, u, u_target, sizes)
        dual_lower, feas, u_reg, primal_upper = terms.unbind(1)
        primal_gap = primal_upper - dual_lower
        loss = weights[0] * primal_gap.mean() + weights[1] * feas.mean() + weights[2] * u_reg.mean()
        ctx.save_for_backward(u, u_target, sizes, weights, ws)
        ctx.in_dtype = u_pred.dtype
        ctx.mark_non_differentiable(primal_gap, dual_lower, feas, u_reg, primal_upper, v_proj, argmin_row, assign, ret)
        return loss, primal_gap, dual_lower, feas, u_reg, primal_upper, v_proj, argmin_row, assign, ret

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, *unused):
        u, u_target, sizes, weights, ws = ctx.saved_tensors
        _hip.require_device()
        B, n = u.shape
        w = (weights * grad_loss.to(torch.float32)).contiguous()
        grad_u = torch.empty_like(u)
        hip_call("lapwarm_train_loss_backward", "train_loss_backward", u.device, B, n, sizes, u, u_target, w, 1.0 / B,
                 grad_u, ws, ws.numel())
        return grad_u.to(ctx.in_dtype), None, None, None, None


def warmstart_loss(cost, u_pred, u_target, mask, weights=DEFAULT_WEIGHTS):
    """The reference's training loss of a padded batch: returns ``(loss, metrics)``.

    cost (B, n, n) float32 and u_target (B, n) float32 on the GPU, u_pred (B, n) float32 (or half precision,
    upcast to float32), mask (B, n) bool, a prefix mask whose row sums are the instance sizes (computed on the
    device; the prefix property is documented, not checked).  `weights` = (primal gap, feas, u_reg), three
    numbers (uploaded once per device and kept) or a float32 tensor of shape (3,) on the GPU.  Only
    u_pred receives a gradient.  `metrics` holds per-instance device tensors: primal_gap, feas, dual_lower,
    primal_upper, u_reg (B,), v_proj (B, n), assign (B, n) int32 with -1 on padded rows, and also argmin_row
    (B, n) int32 and ret (B,) int32 (2 where mask[b] has no row: that instance's terms, and the loss, are
    NaN).  Apart from the first upload of a weights triple nothing is copied from or to the host and nothing
    synchronises: the caller decides when to read them.  Ties: see the module docstring."""
    if u_target is None or mask is None:
        raise TypeError("u_target and mask are required")
    if isinstance(weights, torch.Tensor):
        if weights.dtype != torch.float32 or tuple(weights.shape) != (3,):
            raise ValueError("a weights tensor must be float32 of shape (3,)")
    elif len(weights) != 3:
        raise ValueError("weights must be (primal gap, feas, u_reg)")
    B, n = _check_args(cost, u_pred, u_target, mask)
    cost = cost.contiguous()
    sizes = mask.sum(1, dtype=torch.int32)
    w = _device_weights(weights, cost.device)
    loss, primal_gap, dual_lower, feas, u_reg, primal_upper, v_proj, argmin_row, assign, ret = _WarmstartLoss.apply(
        u_pred, cost, u_target.contiguous(), sizes, w)
    metrics = dict(primal_gap=primal_gap, feas=feas, dual_lower=dual_lower, primal_upper=primal_upper, u_reg=u_reg,
                   v_proj=v_proj, assign=assign, argmin_row=argmin_row, ret=ret)
    return loss, metrics


class _DualWarmstartLoss(torch.autograd.Function):
    """loss = w0 mean(primal_upper - dual_lower) + w1 mean(feas) + w2 mean(v_reg); differentiable in u_pred and
    v_hint.  The backward is one call of lapwarm_dual_loss_backward with grad_scale = 1 / B and the weights
    multiplied by the incoming gradient on the device: nothing is added to what the kernel returns."""

    @staticmethod
    def forward(ctx, u_pred, v_hint, cost, sizes, weights):
        lib = _hip.require_device()
        u = u_pred.detach().to(torch.float32).contiguous()
        vh = v_hint.detach().to(torch.float32).contiguous()
        B, n = u.shape
        dev = cost.device
        v_proj = torch.empty((B, n), dtype=torch.float32, device=dev)
        argmin_row = torch.empty((B, n), dtype=torch.int32, device=dev)
        assign = torch.empty((B, n), dtype=torch.int32, device=dev)
        terms = torch.empty((B, 4), dtype=torch.float32, device=dev)
        ret = torch.empty((B,), dtype=torch.int32, device=dev)
        nbytes = int(lib.lapwarm_dual_loss_workspace_bytes(B, n))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        hip_call("lapwarm_dual_loss_forward", "dual_loss_forward", dev, cost, B, n, sizes, u, vh, v_proj, argmin_row,
                 assign, terms, ret, ws, nbytes)
        dual_lower, feas, v_reg, primal_upper = terms.unbind(1)
        primal_gap = primal_upper - dual_lower
        loss = weights[0] * primal_gap.mean() + weights[1] * feas.mean() + weights[2] * v_reg.mean()
        ctx.save_for_backward(u, vh, sizes, weights, ws)
        ctx.in_dtypes = (u_pred.dtype, v_hint.dtype)
        ctx.mark_non_differentiable(primal_gap, dual_lower, feas, v_reg, primal_upper, v_proj, argmin_row, assign, ret)
        return loss, primal_gap, dual_lower, feas, v_reg, primal_upper, v_proj, argmin_row, assign, ret

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, *unused):
        u, vh, sizes, weights, ws = ctx.saved_tensors
        _hip.require_device()
        B, n = u.shape
        w = (weights * grad_loss.to(torch.float32)).contiguous()
        grad_u = torch.empty_like(u)
        grad_vh = torch.empty_like(vh)
        hip_call("lapwarm_dual_loss_backward", "dual_loss_backward", u.device, B, n, sizes, u, vh, w, 1.0 / B, grad_u,
                 grad_vh, ws, ws.numel())
        return grad_u.to(ctx.in_dtypes[0]), grad_vh.to(ctx.in_dtypes[1]), None, None, None


def dual_warmstart_loss(cost, u_pred, v_hint, mask, weights=DEFAULT_WEIGHTS):
    """The reference's DualGNN training loss (gnn/train.py:267-308) of a padded batch: ``(loss, metrics)``.

    cost (B, n, n) float32 on the GPU; u_pred and v_hint (B, n), the model's two outputs, float32 (or half
    precision, upcast to float32; each gradient comes back in its input's dtype); mask (B, n) bool, a prefix mask
    as in `warmstart_loss`.  `weights` = (primal gap, feas, v_reg), three numbers or a float32 tensor of shape (3,)
    on the GPU.  u_pred and v_hint receive gradients, from one backward kernel.  `metrics` is that of
    `warmstart_loss` with v_reg in place of u_reg.  Apart from the first upload of a weights triple nothing is
    copied from or to the host and nothing synchronises.  Ties: see the module docstring."""
    if v_hint is None or mask is None:
        raise TypeError("v_hint and mask are required")
    if isinstance(weights, torch.Tensor):
        if weights.dtype != torch.float32 or tuple(weights.shape) != (3,):
            raise ValueError("a weights tensor must be float32 of shape (3,)")
    elif len(weights) != 3:
        raise ValueError("weights must be (primal gap, feas, v_reg)")
    _check_args(cost, u_pred, None, mask, v_hint)
    cost = cost.contiguous()
    sizes = mask.sum(1, dtype=torch.int32)
    w = _device_weights(weights, cost.device)
    loss, primal_gap, dual_lower, feas, v_reg, primal_upper, v_proj, argmin_row, assign, ret = _DualWarmstartLoss.apply(
        u_pred, v_hint, cost, sizes, w)
    metrics = dict(primal_gap=primal_gap, feas=feas, dual_lower=dual_lower, primal_upper=primal_upper, v_reg=v_reg,
                   v_proj=v_proj, assign=assign, argmin_row=argmin_row, ret=ret)
    return loss, metrics


@torch.no_grad()
def greedy_primal_upper_batch(cost, u, mask=None):
    """The evaluation metric of the reference's eval.py (`greedy_primal_upper_np`): the greedy assignment on
    the reduced costs of u and its min-trick v.  cost (B, n, n) float32 on the GPU, u (B, n), mask (B, n) bool
    prefix mask or None for full instances.  Returns ``(primal_upper (B,) float32, assign (B, n) int32)``."""
    B, n = _check_args(cost, u, None, mask)
    cost = cost.contiguous()
    if mask is None:
        sizes = torch.full((B,), n, dtype=torch.int32, device=cost.device)
    else:
        sizes = mask.sum(1, dtype=torch.int32)
    u = u.detach().to(torch.float32).contiguous()
    _, _, assign, terms, _, _ = _forward(cost, u, u, sizes)
    return terms[:, 3], assign
