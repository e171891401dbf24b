#!/usr/bin/env python3
"""Time WarmStartPipeline.solve_many (ragged features, OneGNN, min-trick, seeded solve) on the MI355X.

Two cases, one JSON line each; the cost matrices are resident on the device and the seeds are the model's:
  distinct  B instances of B distinct sizes spread evenly over [lo, hi] (uniform family)
  same      B instances of one size n: the case in which grouping by kernel configuration can gain nothing
Each figure is a host-clock mean over `inner` back-to-back solve_many calls after `warmup` untimed ones, with one
device synchronise at the end; `reps` of them are listed, so that the run-to-run spread can be read beside the median.
`--pkg DIR` times another checkout of the package (its own library and Python) with the same inputs: that is
how a baseline is taken in the same session.

Usage:  python tools/bench_solve_many.py [--batch 32] [--lo 384] [--hi 640] [--n 512] [--reps 3] [--inner 10]
                                         [--warmup 5] [--pkg DIR] [--out FILE]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lo", type=int, default=384)
    ap.add_argument("--hi", type=int, default=640)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pkg", default=str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd"))
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.pkg).resolve()))

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_solve_many.py needs the MI355X: nothing here is measured on a CPU")
    from gnn import OneGNN, WarmStartPipeline
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pipe = WarmStartPipeline(OneGNN(21, 64, 2).eval(), dev)
    label = args.label or Path(args.pkg).resolve().parent.name

    def mean_ms(fn):
        for _ in range(args.warmup):  # (one call is not enough: the first timed figures of a process fall)
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.inner

    def run(case, sizes):
        rs = np.random.RandomState(len(sizes) * 1000 + sizes[0])
        costs = [torch.from_numpy(rs.uniform(0.0, 1.0, (m, m))).to(dev) for m in sizes]
        out = pipe.solve_many(costs)
        torch.cuda.synchronize()
        rets = [int(o["ret"]) for o in out]
        digest = int(sum(int(o["x"].sum()) * (b + 1) for b, o in enumerate(out)))  # equal inputs, equal answers
        ms = [mean_ms(lambda: pipe.solve_many(costs)) for _ in range(args.reps)]
        line = dict(case=case, label=label, batch=len(sizes), sizes=[min(sizes), max(sizes)],
                    distinct_sizes=len(set(sizes)), solve_many_ms=[round(t, 3) for t in ms],
                    median_ms=round(float(np.median(ms)), 3), spread_ms=round(max(ms) - min(ms), 3),
                    ret_nonzero=sum(r != 0 for r in rets), x_digest=digest)
        print(json.dumps(line), flush=True)
        return line

    B = args.batch
    lines = [run("distinct", [int(x) for x in np.linspace(args.lo, args.hi, B).round()]),
             run("same", [args.n] * B)]
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
