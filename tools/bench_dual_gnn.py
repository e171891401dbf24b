"""DualGNN forward on the MI355X: the fused path against the plain torch path on the same device, and the graph
features against NumPy on one core.

The CPU side of the features comparison is the reference's own `compute_features` when `--reference DIR` names a
checkout of the reference (its gnn/features.py is loaded by oracle.ref.load_module; with `--cpu-only` nothing else runs and no GPU is
needed, so the CPU figure can come from a host that has the checkout).  Without it the tool times `numpy_features`
below, a PARTIAL formulation (statistics and stable ranks of both sides; no edge-tensor assembly, no positional
encodings, no reduced cost), and labels the figure so.

Resident inputs, warm-up, host-clock means of back-to-back calls between two device synchronisations, three runs
per figure (mean and run-to-run spread), peak allocated memory of one forward.  One JSON line per figure.
Kernel times: run this script under `rocprofv3 --kernel-trace --stats -- python tools/bench_dual_gnn.py --fused-only`
in a run of its own.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gnn.dual_gnn import DualGNN, DualLayer  # noqa: E402
from gnn.features import graph_features_device  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, calls, runs=3, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    means = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        means.append((time.perf_counter() - t0) / calls * 1e3)
    return {"ms": float(np.mean(means)), "spread_ms": float(max(means) - min(means)), "runs": means}


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(DEV) - base) / 2 ** 20


def numpy_features(C):
    """A partial NumPy formulation of compute_features: the statistics and stable ranks of both sides, without the
    (n, n, 10) edge assembly, the positional encodings and the reduced cost.  Not a bound on the full function in either direction: its two stable argsorts per side cost
    more than the reference's default argsort."""
    n = C.shape[0]
    out = []
    for M in (C, C.T):
        med = np.median(M, axis=1)
        mad = np.maximum(np.median(np.abs(M - med[:, None]), axis=1), 1e-9)
        e = np.exp(-M)
        p = e / (e.sum(axis=1, keepdims=True) + 1e-9)
        ent = -(p * np.log(p + 1e-9)).sum(axis=1)
        rank = np.argsort(np.argsort(M, axis=1, kind="stable"), axis=1, kind="stable") / max(1, n - 1)
        gap = M - M.min(axis=1, keepdims=True)
        out.append((med, mad, ent, rank, gap, (gap <= 1e-3).mean(axis=1), M.max(axis=1), M.mean(axis=1), M.std(axis=1)))
    return out


def cpu_features_ms(reference, n=512, runs=3):
    """One-core time of the features at n: the reference's compute_features if a checkout is given."""
    torch.set_num_threads(1)
    fn, what = numpy_features, "partial NumPy formulation (numpy_features)"
    if reference:
        from oracle.ref import load_module
        mod = load_module("gnn/features.py", "_ref_features", root=reference)
        fn, what = mod.compute_features, "reference compute_features"
    C = np.random.default_rng(1).random((n, n)) * 10.0
    fn(C)
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn(C)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"what": "features_cpu", "n": n, "cpu_side": what, "one_core_ms": float(np.mean(ms)),
            "spread_ms": float(max(ms) - min(ms)), "runs": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--reference", default=None, help="checkout of the reference, for the CPU side of the features")
    ap.add_argument("--cpu-only", action="store_true", help="only the one-core CPU time of the features")
    ap.add_argument("--shapes", default="8x256,1x512,1x1024")
    args = ap.parse_args()
    if args.cpu_only:
        print(json.dumps(cpu_features_ms(args.reference)), flush=True)
        return
    torch.manual_seed(0)
    model = DualGNN(hidden_dim=128, layers=4, heads=4).to(DEV).eval()
    rng = np.random.default_rng(0)
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        C = torch.from_numpy(rng.random((B, n, n)) * 10.0).to(DEV)
        edge, row, col = graph_features_device(C)

        def fused():
            with torch.no_grad():
                return model(edge, row, col)

        def plain():  # the plain torch path of the same module, without recording a gradient
            keep = DualLayer.takes_fused_path
            DualLayer.takes_fused_path = lambda *a: False
            try:
                with torch.no_grad():
                    return model(edge, row, col)
            finally:
                DualLayer.takes_fused_path = keep

        calls = 10 if n <= 512 else 4
        rec = {"what": "forward", "B": B, "n": n, "fused": timed(fused, calls), "fused_peak_MiB": peak_mib(fused)}
        if not args.fused_only:
            try:
                rec["plain"] = timed(plain, max(1, calls // 4), warmup=1)
                rec["plain_peak_MiB"] = peak_mib(plain)
            except torch.OutOfMemoryError:
                rec["plain"] = "out of memory"
        rec["features"] = timed(lambda: graph_features_device(C), calls)
        print(json.dumps(rec), flush=True)
    if not args.fused_only:
        print(json.dumps(cpu_features_ms(args.reference)), flush=True)
        Cd = torch.from_numpy(rng.random((512, 512)) * 10.0).to(DEV)
        print(json.dumps({"what": "features", "n": 512, "device": timed(lambda: graph_features_device(Cd), 20)}),
              flush=True)


if __name__ == "__main__":
    main()
