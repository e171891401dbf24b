#!/usr/bin/env python3
"""Time the device training loss (gnn.losses.warmstart_loss, forward + backward) on the MI355X.

At B = 32 and n in {512, 2048} (uniform float32 costs, u_pred = a random perturbation of the row-minimum
duals): the device loss, and beside it the same loss the way a training script without these kernels computes
it: the formula of DESIGN.md composed from torch ops on the same device, (B, n, n) temporaries and autograd
included, with the greedy bound on the host, one instance at a time, an `np.argsort` per row.  Both are timed
with a host clock around work that ends in a device synchronise, alternating, after a warm-up of each; the
device figure is the mean of 50 back-to-back steps, so it includes the step's allocations.  Prints one JSON line
per size; `composed_host_greedy_ms` is the part of the composed time spent in the host greedy, copies included.

With --dual the loss is DualGNN's (gnn.losses.dual_warmstart_loss: v_reg on a v_hint, two gradients) and the
composed formula has its third term; `onegnn_device_ms` is then the OneGNN device loss on the same costs in the
same run, 50 back-to-back steps as well: the dual loss should cost that plus the per-row segment sum.

Usage:  python tools/bench_train_loss.py [--reps 5] [--sizes 512 2048] [--dual] [--out FILE]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def greedy_on_host(cost, reduced):
    """The greedy bound of one instance on the host, from its definition: rows in ascending order of their
    smallest reduced cost, each takes its cheapest column that is still free.  NumPy's default (unstable)
    argsort ranks the rows and, per row, the columns, which is the work the host greedy of the reference spends
    its time in; picking the first free column of a ranking is vectorised here, so this baseline is, if
    anything, quicker than a Python loop over the ranking."""
    n = cost.shape[0]
    free = np.ones(n, dtype=bool)
    taken = np.empty(n, dtype=np.int64)
    for r in np.argsort(reduced.min(axis=1)):
        ranking = np.argsort(reduced[r])
        j = ranking[free[ranking]][0]
        free[j] = False
        taken[r] = j
    return float(cost[np.arange(n), taken].sum(dtype=np.float64))


def composed_loss(cost, u_pred, u_target, mask, clock, weights=(1.0, 1.0, 0.1), v_hint=None):
    """The loss of DESIGN.md's table (section "Training loss") in torch ops on the tensors' device, float32
    throughout, with (B, n, n) temporaries and autograd doing the backward; the greedy bound is computed on
    the host, one instance at a time, from copies of C and the reduced costs.  clock["greedy"] collects the
    time of that host part, copies included.  With v_hint the third term is DualGNN's v_reg on it."""
    B, n = u_pred.shape
    sizes = mask.sum(dim=1)
    pair = mask[:, :, None] & mask[:, None, :]
    inf = torch.full((), float("inf"), dtype=cost.dtype, device=cost.device)
    zero = torch.zeros((), dtype=cost.dtype, device=cost.device)
    shifted = cost - u_pred[:, :, None]                                  # C_ij - u_i
    v = torch.where(pair, shifted, inf).amin(dim=1)                      # v_j over the valid rows
    v = torch.where(mask, v, zero)
    dual_lower = torch.where(mask, u_pred, zero).sum(dim=1) + v.sum(dim=1)
    residue = ((u_pred[:, :, None] + v[:, None, :]) - cost).clamp_min(0.0)
    feas = torch.where(pair, residue, zero).sum(dim=(1, 2)) / (sizes * sizes).to(cost.dtype)
    if v_hint is None:
        u_reg = torch.where(mask, (u_pred - u_target).square(), zero).sum(dim=1) / sizes.to(cost.dtype)
    else:
        u_reg = torch.where(mask, (v_hint - v).square(), zero).sum(dim=1) / sizes.to(cost.dtype)
    reduced = (shifted - v[:, None, :]).detach()
    t0 = time.perf_counter()
    host_sizes = sizes.tolist()
    primal_upper = torch.tensor(
        [greedy_on_host(cost[b, :k, :k].cpu().numpy(), reduced[b, :k, :k].cpu().numpy())
         for b, k in enumerate(host_sizes)], dtype=cost.dtype).to(cost.device)
    clock["greedy"] += time.perf_counter() - t0
    w0, w1, w2 = weights
    loss = w0 * (primal_upper - dual_lower).mean() + w1 * feas.mean() + w2 * u_reg.mean()
    return loss, primal_upper


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--dual", action="store_true", help="time dual_warmstart_loss, the OneGNN loss beside it")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gnn.losses import dual_warmstart_loss, warmstart_loss
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_loss.py needs the MI355X: nothing here is measured on a CPU")
    dev = torch.device("cuda:0")
    lines = []
    for n in args.sizes:
        B = args.batch
        g = torch.Generator(device=dev).manual_seed(n)
        cost = torch.rand((B, n, n), dtype=torch.float32, device=dev, generator=g)
        u_target = cost.min(dim=2).values
        u0 = u_target + 0.05 * torch.randn((B, n), dtype=torch.float32, device=dev, generator=g)
        mask = torch.ones((B, n), dtype=torch.bool, device=dev)
        # --dual: v_hint = a random perturbation of the min-trick of u_target
        v0 = (cost - u_target[:, :, None]).amin(dim=1) + 0.05 * torch.randn((B, n), dtype=torch.float32, device=dev,
                                                                            generator=g) if args.dual else None
        clock = {"greedy": 0.0}

        def onegnn_step():
            u = u0.clone().requires_grad_()
            loss, metrics = warmstart_loss(cost, u, u_target, mask)
            loss.backward()
            return loss.detach(), u.grad, metrics["primal_upper"]

        def dual_step():
            u, vh = u0.clone().requires_grad_(), v0.clone().requires_grad_()
            loss, metrics = dual_warmstart_loss(cost, u, vh, mask)
            loss.backward()
            return loss.detach(), (u.grad, vh.grad), metrics["primal_upper"]

        def composed_step():
            u = u0.clone().requires_grad_()
            vh = v0.clone().requires_grad_() if args.dual else None
            loss, primal = composed_loss(cost, u, u_target, mask, clock, v_hint=vh)
            loss.backward()
            return loss.detach(), (u.grad, vh.grad) if args.dual else u.grad, primal

        device_step = dual_step if args.dual else onegnn_step

        timed(device_step)
        timed(composed_step)
        clock["greedy"] = 0.0
        t_dev, t_ref = [], []
        for _ in range(args.reps):
            ms, (loss_d, grad_d, primal_d) = timed(device_step)
            t_dev.append(ms)
            ms, (loss_c, grad_c, primal_c) = timed(composed_step)
            t_ref.append(ms)
        # a long window of the device step alone: one step is too short for a host clock
        inner = 50
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            device_step()
        torch.cuda.synchronize()
        dev_ms = (time.perf_counter() - t0) * 1e3 / inner
        line = dict(batch=B, n=n, device_ms=round(dev_ms, 4), device_single_ms_median=round(float(np.median(t_dev)), 4),
                    composed_ms_median=round(float(np.median(t_ref)), 2), composed_ms_min=round(min(t_ref), 2),
                    composed_host_greedy_ms=round(clock["greedy"] * 1e3 / args.reps, 2),
                    speedup=round(float(np.median(t_ref)) / dev_ms, 1),
                    loss_device=float(loss_d), loss_composed=float(loss_c),
                    primal_equal=int((primal_d == primal_c).sum()),
                    C_GBps_two_reads=round(2 * B * n * n * 4 / (dev_ms * 1e-3) / 1e9, 1))
        if args.dual:
            line["loss"] = "dual"
            line["grad_max_abs_diff"] = float((grad_d[0] - grad_c[0]).abs().max())
            line["grad_v_hint_max_abs_diff"] = float((grad_d[1] - grad_c[1]).abs().max())
            onegnn_step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                onegnn_step()
            torch.cuda.synchronize()
            line["onegnn_device_ms"] = round((time.perf_counter() - t0) * 1e3 / inner, 4)
        else:
            line["grad_max_abs_diff"] = float((grad_d - grad_c).abs().max())
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
