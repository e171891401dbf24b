#!/usr/bin/env python3
"""Time DualWarmStartPipeline.predict_ragged (ragged graph features, one DualGNN forward with sizes, min-trick) on
the MI355X against the two ways to get the same predictions without it.

Two workloads, one JSON line each; the cost matrices are resident on the device:
  distinct  B instances of B distinct sizes spread evenly over [lo, hi] (uniform family).  Three paths:
              ragged   predict_ragged
              loop     one predict_batch call per instance (every size is its own uniform batch)
              padded   the same padded forward through the uniform kernels with the prefix mask (sizes=None)
            and the two edge-score entries alone on the padded features of the batch, whose time ratio stands beside
            the share of real edges, sum n_b^2 / (B N^2)
  same      B instances of one size n, where nothing can be gained: predict_ragged against one predict_batch
Each figure is a host-clock mean over `inner` back-to-back calls after `warmup` untimed ones, with one device
synchronise at the end; `reps` rounds are listed, the paths alternating inside a round, so that the run-to-run spread
can be read beside the median.

Usage:  python tools/bench_dual_ragged.py [--batch 32] [--lo 384] [--hi 640] [--n 512] [--hidden 128] [--layers 4]
                                          [--heads 4] [--reps 3] [--inner 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lo", type=int, default=384)
    ap.add_argument("--hi", type=int, default=640)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dual_ragged.py needs the MI355X: nothing here is measured on a CPU")
    from gnn._call import hip_call
    from gnn.dual_gnn import DualGNN
    from gnn.features import graph_features_packed, min_trick_ragged, ragged_pack
    from gnn.pipeline import DualWarmStartPipeline, _centre_per_instance
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = DualGNN(hidden_dim=args.hidden, layers=args.layers, heads=args.heads).eval()
    pipe = DualWarmStartPipeline(model, dev)

    def mean_ms(fn, inner=args.inner):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / inner

    def timed(paths):
        """{name: [ms per round]}, the paths alternating inside every round, and the summary fields of each"""
        ms = {name: [] for name in paths}
        with torch.inference_mode():
            for _ in range(args.reps):
                for name, fn in paths.items():
                    ms[name].append(mean_ms(fn))
        out = {}
        for name, t in ms.items():
            out[f"{name}_ms"] = [round(x, 3) for x in t]
            out[f"{name}_median_ms"] = round(float(np.median(t)), 3)
            out[f"{name}_spread_ms"] = round(max(t) - min(t), 3)
        return out

    def costs_of(sizes):
        rs = np.random.RandomState(len(sizes) * 1000 + sizes[0])
        return [torch.from_numpy(rs.uniform(0.0, 1.0, (m, m))).to(dev) for m in sizes]

    def padded_uniform(costs):
        """predict_ragged through the uniform kernels: the prefix mask in place of the sizes"""
        pack = ragged_pack(costs, dev)
        f = graph_features_packed(pack)
        u = pipe.model(f.edge, f.row, f.col, f.mask)["u"].to(torch.float64)
        u = _centre_per_instance(u, pack.sizes, f.mask)
        return u, min_trick_ragged(pack, u)

    def edge_scores_alone(costs):
        """the two edge-score entries on the padded features of the batch, first layer's weights"""
        pack = ragged_pack(costs, dev)
        f = graph_features_packed(pack)
        B, N, H = len(pack.host_sizes), pack.N, args.heads
        layer = pipe.model.layers[0]
        lin1, lin2 = layer.edge_mlp[0], layer.edge_mlp[3]
        G = torch.rand((2 * H, 128), device=dev) - 0.5
        scores = torch.empty((B, 2, H, N, N), dtype=torch.float32, device=dev)
        w = (f.edge, lin1.weight, lin1.bias, lin2.weight, lin2.bias, G, scores)
        return timed({
            "edge_scores_uniform": lambda: hip_call("lapwarm_dual_edge_scores", "bench", dev, *w, B, N, H),
            "edge_scores_ragged": lambda: hip_call("lapwarm_dual_edge_scores_ragged", "bench", dev, *w, pack.sizes, B, N,
                                                   H)})

    def worst_gap(got, want):
        return max(float((g.double() - w.double()).abs().max()) for g, w in zip(got, want))

    lines = []
    B = args.batch
    sizes = [int(x) for x in np.linspace(args.lo, args.hi, B).round()]
    costs = costs_of(sizes)
    with torch.inference_mode():
        ragged = [u for u, _ in pipe.predict_ragged(costs)]
        loop = [pipe.predict_batch(c[None])[0][0] for c in costs]
        pu, _ = padded_uniform(costs)
    line = dict(case="distinct", batch=B, sizes=[min(sizes), max(sizes)], distinct_sizes=len(set(sizes)),
                hidden=args.hidden, layers=args.layers, heads=args.heads,
                real_edge_share=round(sum(m * m for m in sizes) / (B * max(sizes) ** 2), 4),
                ragged_vs_loop_max_abs_u=worst_gap(ragged, loop),
                ragged_equals_padded=all(torch.equal(r, pu[b, :m]) for b, (r, m) in enumerate(zip(ragged, sizes))))
    line.update(timed({"ragged": lambda: pipe.predict_ragged(costs),
                       "loop": lambda: [pipe.predict_batch(c[None]) for c in costs],
                       "padded": lambda: padded_uniform(costs)}))
    line.update(edge_scores_alone(costs))
    line["edge_scores_time_ratio"] = round(line["edge_scores_ragged_median_ms"] / line["edge_scores_uniform_median_ms"], 4)
    print(json.dumps(line), flush=True)
    lines.append(line)
    del costs, ragged, loop, pu

    same = costs_of([args.n] * B)
    stacked = torch.stack(same)
    with torch.inference_mode():
        ragged = torch.stack([u for u, _ in pipe.predict_ragged(same)])
        batch_u = pipe.predict_batch(stacked)[0]
    line = dict(case="same", batch=B, sizes=[args.n, args.n], distinct_sizes=1, hidden=args.hidden, layers=args.layers,
                heads=args.heads, real_edge_share=1.0, ragged_vs_batch_max_abs_u=worst_gap([ragged], [batch_u]))
    line.update(timed({"ragged": lambda: pipe.predict_ragged(same), "batch": lambda: pipe.predict_batch(stacked)}))
    print(json.dumps(line), flush=True)
    lines.append(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
