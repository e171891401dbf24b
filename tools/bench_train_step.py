#!/usr/bin/env python3
"""Time one OneGNN training step on the MI355X with the refinement in the reference's op order
(`fused_refine_training = False`, the default) and fused (`True`: HIP aggregation forward and backward).

A step is: model forward in training mode with `topk_values=`, `gnn.losses.warmstart_loss`, backward.  The row
features and the top-16 costs are computed once, outside the step.  Both variants run in one process on the
same inputs and the same weights (hidden 192, 4 layers, dropout 0.1), alternating, after a warm-up of each; the
figure is the host-clock mean of back-to-back steps that end in one device synchronise, so it includes the
step's allocations.  Beside it: `torch.cuda.max_memory_allocated` over the steps of each variant (the inputs,
which both share, included), and the largest difference between the two variants' parameter gradients with
dropout off, as a check that the same thing was timed.  Prints one JSON line per size.

Usage:  python tools/bench_train_step.py [--steps 20] [--sizes 2048 512] [--out FILE]
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

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=192)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gnn import OneGNN
    from gnn.features import row_features_device
    from gnn.losses import warmstart_loss
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_step.py needs the MI355X: nothing here is measured on a CPU")
    dev = torch.device("cuda:0")
    lines = []
    for n in args.sizes:
        B, H = args.batch, args.hidden
        g = torch.Generator(device=dev).manual_seed(n)
        cost = torch.rand((B, n, n), dtype=torch.float32, device=dev, generator=g)
        feat, topk = row_features_device(cost.to(torch.float64))
        u_target = cost.min(dim=2).values
        mask = torch.ones((B, n), dtype=torch.bool, device=dev)
        torch.manual_seed(0)
        model = OneGNN(feat.shape[-1], hidden=H, layers=args.layers, dropout=0.1).to(dev).train()

        def step(fused):
            model.fused_refine_training = fused
            model.zero_grad(set_to_none=True)
            u = model(feat, topk_values=topk, mask=mask)["u"]
            loss, _ = warmstart_loss(cost, u, u_target, mask)
            loss.backward()
            return loss.detach()

        def window(fused):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(fused)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.steps, torch.cuda.max_memory_allocated(dev)

        # the same thing is computed: gradients of the two variants with dropout off
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        grads = {}
        for fused in (False, True):
            step(fused)
            grads[fused] = {k: p.grad.clone() for k, p in model.named_parameters()}
        diff = max(float((grads[True][k] - grads[False][k]).abs().max()) for k in grads[True])
        scale = max(float(v.abs().max()) for v in grads[False].values())
        del grads
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.1

        held = torch.cuda.memory_allocated(dev)
        for fused in (False, True):
            for _ in range(args.warmup):
                step(fused)
        ms = {False: [], True: []}
        peak = {False: 0, True: 0}
        for _ in range(args.rounds):
            for fused in (False, True):
                t, m = window(fused)
                ms[fused].append(t)
                peak[fused] = max(peak[fused], m)
        ref_ms, fused_ms = min(ms[False]), min(ms[True])
        line = dict(batch=B, n=n, hidden=H, layers=args.layers, steps=args.steps, rounds=args.rounds,
                    reference_order_ms=round(ref_ms, 3), fused_ms=round(fused_ms, 3),
                    reference_order_ms_all=[round(x, 3) for x in ms[False]],
                    fused_ms_all=[round(x, 3) for x in ms[True]],
                    speedup=round(ref_ms / fused_ms, 2),
                    reference_order_peak_MB=round(peak[False] / 1e6, 1), fused_peak_MB=round(peak[True] / 1e6, 1),
                    peak_saved_MB=round((peak[False] - peak[True]) / 1e6, 1),
                    inputs_and_weights_MB=round(held / 1e6, 1),
                    edge_tensor_MB=round(B * n * 16 * H * 4 / 1e6, 1),
                    grad_max_abs_diff=diff, grad_max_abs=scale)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del cost, feat, topk, u_target, mask, model
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
