#!/usr/bin/env python3
"""Time the oracle duals of a mixed-size batch on the MI355X: one WarmStartPipeline.oracle_duals_many call (one
lapwarm_oracle_duals_ragged launch chain) against the loop of per-instance oracle_duals_batch calls.

Two cases, one JSON line each; the cost matrices and the matchings (cold lapjv, computed once) are resident on the
device:
  distinct  B instances of B distinct sizes spread evenly over [lo, hi] (uniform family)
  same      B instances of one size n: nothing can be gained over ONE uniform oracle_duals_batch call on the
            stacked batch, which is timed as well
`ragged` is the whole oracle_duals_many call, packing included (distinct: a list of matrices and matchings, packed
on the device; same: the stacked block and matching the uniform call gets, read in place); `ragged_packed` is
oracle_duals_ragged on a pack made once.  Like the uniform call, oracle_duals_many hands back padded device
tensors; the per-instance views of its result are made when they are read, outside the timed calls.
Each figure is a host-clock mean over `inner` back-to-back calls after `warmup` untimed ones, with one device
synchronise at the end; `reps` of them are listed, so that the run-to-run spread can be read beside the median.
`--pkg DIR` times another checkout of the package (its own library and Python) with the same inputs; a checkout
without oracle_duals_many reports the loop and the uniform call only: that is how a baseline is taken in the same
session.

Usage:  python tools/bench_oracle_ragged.py [--batch 32] [--lo 384] [--hi 640] [--n 512] [--reps 3] [--inner 10]
                                            [--warmup 3] [--pkg DIR] [--out FILE]
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pkg", default=str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd"))
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.pkg).resolve()))

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_oracle_ragged.py needs the MI355X: nothing here is measured on a CPU")
    from gnn import OneGNN, WarmStartPipeline
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pipe = WarmStartPipeline(OneGNN(21, 64, 2).eval(), dev)
    label = args.label or Path(args.pkg).resolve().parent.name
    has_many = hasattr(pipe, "oracle_duals_many")

    def times(fn):
        out = []
        for _ in range(args.reps):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / args.inner)
        return out

    def stats(name, ms):
        return {f"{name}_ms": [round(t, 3) for t in ms], f"{name}_median_ms": round(float(np.median(ms)), 3),
                f"{name}_spread_ms": round(max(ms) - min(ms), 3)}

    def run(case, sizes):
        rs = np.random.RandomState(len(sizes) * 1000 + sizes[0])
        costs = [torch.from_numpy(rs.uniform(0.0, 1.0, (m, m))).to(dev) for m in sizes]
        singles = [c.unsqueeze(0) for c in costs]
        xs = [pipe.lapjv_batch(c, want_stats=False)[0] for c in singles]  # (1, n) int32 each

        def loop():
            return [pipe.oracle_duals_batch(c, x) for c, x in zip(singles, xs)]

        ref = loop()
        torch.cuda.synchronize()
        line = dict(case=case, label=label, batch=len(sizes), sizes=[min(sizes), max(sizes)],
                    distinct_sizes=len(set(sizes)), ret_nonzero=sum(int(r[3][0]) != 0 for r in ref))
        line.update(stats("loop", times(loop)))
        if len(set(sizes)) == 1:
            stacked, xst = torch.stack(costs), torch.cat(xs)
            line.update(stats("uniform", times(lambda: pipe.oracle_duals_batch(stacked, xst))))
        if has_many:
            xl = [x[0] for x in xs]
            same = len(set(sizes)) == 1

            def many():  # same size: what the uniform call is given, the stacked block and matching, read in place
                return pipe.oracle_duals_many(stacked, xst) if same else pipe.oracle_duals_many(costs, xl)

            got = many()
            torch.cuda.synchronize()
            line["bit_equal_to_loop"] = all(
                torch.equal(g[1].view(torch.int64), r[1][0].view(torch.int64)) and
                torch.equal(g[2].view(torch.int64), r[2][0].view(torch.int64)) and
                torch.equal(g[4], r[4][0]) for g, r in zip(got, ref))
            line.update(stats("ragged", times(many)))
            line["loop_over_ragged"] = round(line["loop_median_ms"] / line["ragged_median_ms"], 2)
            # the same without the pack: a caller that keeps its ragged_pack (training_batch does) pays this
            from gnn.features import ragged_pack
            pack = ragged_pack(costs, dev)
            xp = torch.nn.utils.rnn.pad_sequence(xl, batch_first=True, padding_value=-1)  # int32, as the uniform call's
            line.update(stats("ragged_packed", times(lambda: pipe.oracle_duals_ragged(pack, xp))))
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
