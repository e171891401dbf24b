#!/usr/bin/env python3
"""Synthetic cost families made on the MI355X (gnn.synthetic.synthetic_pack) against the two things they can be
held to, in the same run, one JSON line per case:

  host    the only route before the device generator: solvers.generators.generate_family per instance (NumPy, one
          thread) and one gnn.ragged_pack of the results (one upload)
  fill    a plain device fill of the same number of bytes (torch.Tensor.fill_ of the pack's buffer): what writing
          the batch costs when nothing is computed, the write roofline of the generator

Cases: each of the seven families and the K3 mix (uniform, sparse, metric, clustered, a quarter of the batch each),
at `--batch` instances of `--n` and at `--batch` distinct sizes spread evenly over [--lo, --hi].  A last line compares
WarmStartPipeline.synthetic_training_batch with training_batch on host-made costs for the distinct-size K3 mix.

Each figure is a host-clock mean over `inner` back-to-back calls after `warmup` untimed ones with one device
synchronise at the end (synthetic_pack itself reads its return codes back, so it is synchronous anyway); `reps` of
them are listed with their median and spread (max - min).  The host route is timed once per rep (inner = 1).

Usage:  python tools/bench_cost_families.py [--batch 32] [--n 2048] [--lo 384] [--hi 640] [--reps 5] [--inner 10]
                                            [--warmup 2] [--host-reps 3] [--out FILE]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
FAMILIES = ("uniform", "metric", "low_rank", "clustered", "noisy_linear", "tie", "sparse")
K3 = ("uniform", "sparse", "metric", "clustered")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--lo", type=int, default=384)
    ap.add_argument("--hi", type=int, default=640)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd"))

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cost_families.py needs the MI355X: nothing here is measured on a CPU")
    from gnn import OneGNN, WarmStartPipeline, ragged_pack, synthetic_pack
    from solvers.generators import generate_family
    dev = torch.device("cuda:0")
    lines = []

    def times(fn, reps, inner, warmup):
        out = []
        for _ in range(reps):
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / inner)
        return out

    def stats(name, ms):
        return {f"{name}_ms": [round(t, 3) for t in ms], f"{name}_median_ms": round(float(np.median(ms)), 3),
                f"{name}_spread_ms": round(max(ms) - min(ms), 3)}

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    def plan(case, sizes):
        B = len(sizes)
        names = [K3[(b * len(K3)) // B] for b in range(B)] if case == "k3_mix" else [case] * B
        seeds = [int(s) for s in np.random.default_rng(1234).integers(0, 2**32 - 1, size=B)]
        return names, list(sizes), seeds

    def run(case, shape, sizes):
        names, sizes, seeds = plan(case, sizes)
        pack = synthetic_pack(names, sizes, seeds, dev)
        nbytes = pack.C.numel() * 8
        line = dict(case=case, shape=shape, batch=len(sizes), sizes=[min(sizes), max(sizes)],
                    mbytes=round(nbytes / 1e6, 1))
        line.update(stats("device", times(lambda: synthetic_pack(names, sizes, seeds, dev), args.reps, args.inner,
                                          args.warmup)))
        buf = torch.empty_like(pack.C)
        line.update(stats("fill", times(lambda: buf.fill_(0.5), args.reps, 10 * args.inner, args.warmup)))

        def host():
            return ragged_pack([generate_family(f, n, s) for f, n, s in zip(names, sizes, seeds)], dev)

        line.update(stats("host", times(host, args.host_reps, 1, 1)))
        line["device_gbytes_per_s"] = round(nbytes / line["device_median_ms"] / 1e6, 1)
        line["fill_gbytes_per_s"] = round(nbytes / line["fill_median_ms"] / 1e6, 1)
        line["device_over_fill"] = round(line["device_median_ms"] / line["fill_median_ms"], 2)
        line["host_over_device"] = round(line["host_median_ms"] / line["device_median_ms"], 1)
        emit(line)

    distinct = [int(x) for x in np.linspace(args.lo, args.hi, args.batch).round()]
    for case in FAMILIES + ("k3_mix",):
        run(case, "same", [args.n] * args.batch)
        run(case, "distinct", distinct)

    torch.manual_seed(0)
    pipe = WarmStartPipeline(OneGNN(21, 64, 2).eval(), dev)
    names, sizes, seeds = plan("k3_mix", distinct)

    def host_batch():
        return pipe.training_batch([generate_family(f, n, s) for f, n, s in zip(names, sizes, seeds)])

    line = dict(case="training_batch", shape="distinct", batch=len(sizes), sizes=[min(sizes), max(sizes)])
    line.update(stats("synthetic_training_batch", times(lambda: pipe.synthetic_training_batch(names, sizes, seeds),
                                                        args.reps, args.inner, args.warmup)))
    line.update(stats("host_training_batch", times(host_batch, args.host_reps, 1, 1)))
    line["host_over_synthetic"] = round(line["host_training_batch_median_ms"] /
                                        line["synthetic_training_batch_median_ms"], 1)
    emit(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
