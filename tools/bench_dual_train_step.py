#!/usr/bin/env python
"""One DualGNN training step on the MI355X, fused attention backward against the plain torch path.

A step is the forward in training mode (dropout 0.1), a scalar of the outputs (mean squared distance of u and
v_hint to fixed random targets over the real nodes, the shape of a warm-start loss without its solver part) and the
backward; no optimiser.  Hidden 128, 4 layers, 4 heads at B = 8 x n = 256, B = 1 x n = 512, B = 1 x n = 1024 and the
32 instances of sizes 384..640 of tools/bench_dual_ragged.py (padded, with `sizes`).  The two paths alternate inside
every round; medians and spreads (max - min) over the rounds, and torch.cuda.max_memory_allocated over a step
relative to what was allocated before it.  A path that runs out of memory is recorded as such.  Per-kernel times come
from a separate run of this file with --only fused under `rocprofv3 --kernel-trace --stats`.

With --loss the scalar is the reference's DualGNN training loss on the device (gnn.losses.dual_warmstart_loss on the
float32 costs of the case): the measured step is forward, loss with its greedy, backward.

With --fused-dropout P a third path, fused_dropout, alternates with the other two: the fused path with
DualGNN.fused_dropout on and p = P in the edge MLP and on the attention weights (the reference's training regime at
P = 0.1); `fused` stays the fused path with the switch off.

Usage:  python tools/bench_dual_train_step.py [--reps 5] [--inner 3] [--only fused|plain] [--cases a,b] [--loss]
                                              [--fused-dropout P] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", choices=("fused", "plain"), default=None)
    ap.add_argument("--cases", default="8x256,1x512,1x1024,ragged")
    ap.add_argument("--loss", action="store_true", help="the step's scalar is dual_warmstart_loss")
    ap.add_argument("--fused-dropout", type=float, default=None, metavar="P",
                    help="also measure the fused path with fused_dropout at this p")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dual_train_step.py needs the MI355X: nothing here is measured on a CPU")
    from gnn.dual_gnn import DualGNN
    from gnn.features import graph_features_device, graph_features_packed, ragged_pack, row_features_packed
    from gnn.losses import dual_warmstart_loss
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = DualGNN(hidden_dim=args.hidden, layers=args.layers, heads=args.heads).to(dev).train()
    if args.fused_dropout is not None:  # the two dropouts of the fused region; fused_dropout switches them per step
        for layer in model.layers:
            layer.edge_mlp[2].p = layer.dropout.p = args.fused_dropout

    def inputs(case):
        rs = np.random.RandomState(len(case))
        if case == "ragged":
            sizes = [int(x) for x in np.linspace(384, 640, 32).round()]
            pack = ragged_pack([torch.from_numpy(rs.uniform(0.0, 1.0, (m, m))).to(dev) for m in sizes], dev)
            f = graph_features_packed(pack)
            cost = row_features_packed(pack, return_topk=False, want_cost32=True).cost32 if args.loss else None
            return f.edge, f.row, f.col, f.mask, pack.sizes, cost
        B, n = (int(x) for x in case.split("x"))
        C = torch.from_numpy(rs.uniform(0.0, 1.0, (B, n, n))).to(dev)
        edge, row, col = graph_features_device(C)
        return edge, row, col, None, None, C.to(torch.float32) if args.loss else None

    lines = []
    for case in args.cases.split(","):
        edge, row, col, mask, sizes, cost = inputs(case)
        g = torch.Generator(device=dev).manual_seed(1)
        tu, tv = (torch.randn(edge.shape[:2], device=dev, generator=g) for _ in range(2))
        keep = torch.ones_like(tu) if mask is None else mask.to(tu.dtype)
        keep_bool = keep.to(torch.bool)

        def step(fused, dropout=False):
            model.fused_attention_training = fused
            model.fused_dropout = dropout
            model.zero_grad(set_to_none=True)
            out = model(edge, row, col, mask, sizes=sizes if fused else None)
            if args.loss:
                loss, _ = dual_warmstart_loss(cost, out["u"], out["v_hint"], keep_bool)
            else:
                loss = (((out["u"] - tu) ** 2 + (out["v_hint"] - tv) ** 2) * keep).sum() / keep.sum()
            loss.backward()

        def measure(fused, dropout=False):
            """(ms per step, peak bytes over a step) or the text of the failure"""
            try:
                for _ in range(args.warmup):
                    step(fused, dropout)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    step(fused, dropout)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / args.inner, torch.cuda.max_memory_allocated() - before
            except torch.OutOfMemoryError as e:
                model.zero_grad(set_to_none=True)
                torch.cuda.empty_cache()
                return str(e).splitlines()[0]

        paths = [p for p in ("fused", "plain") if args.only in (None, p)]
        if args.fused_dropout is not None and "fused" in paths:
            paths.insert(1, "fused_dropout")
        got = {p: [] for p in paths}
        for _ in range(args.reps):
            for p in paths:
                if not got[p] or not isinstance(got[p][-1], str):  # a path that ran out of memory is not tried again
                    got[p].append(measure(p != "plain", p == "fused_dropout"))
        line = dict(case=case, shape=list(edge.shape[:2]), hidden=args.hidden, layers=args.layers, heads=args.heads,
                    reps=args.reps, inner=args.inner, scalar="dual_warmstart_loss" if args.loss else "mse")
        if args.fused_dropout is not None:
            line["fused_dropout_p"] = args.fused_dropout
        for p in paths:
            if isinstance(got[p][-1], str):
                line[f"{p}_failed"] = got[p][-1]
                continue
            ms = [m for m, _ in got[p]]
            line[f"{p}_ms"] = [round(m, 3) for m in ms]
            line[f"{p}_median_ms"] = round(float(np.median(ms)), 3)
            line[f"{p}_spread_ms"] = round(max(ms) - min(ms), 3)
            line[f"{p}_peak_mib"] = round(max(b for _, b in got[p]) / 2**20, 1)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del edge, row, col, tu, tv, keep, cost
        model.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
