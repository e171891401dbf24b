#!/usr/bin/env python3
"""Time the batched oracle duals (WarmStartPipeline.oracle_duals_batch) on the MI355X.

For (32, 2048) per family and (1, 16384) uniform: the whole call with a given matching, the cold
lapjv_batch that produces the matching, and lapwarm_colmin_batched on the same batch as a
bandwidth yardstick (one read of C).  Prints one JSON line per configuration: sweeps, rows read,
ms, and the bytes per second of the sweeps (rows read * n * 8 B over the oracle call's time, an
under-estimate: the call also holds the final reduced-cost pass and the host round trips).

Usage:  python tools/bench_oracle_duals.py [--reps 5] [--out FILE]
"""
import argparse
import ctypes as ct
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


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gnn import OneGNN, WarmStartPipeline
    from solvers.generators import generate_family
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pipe = WarmStartPipeline(OneGNN(21, hidden=32, layers=1).eval(), dev)
    lib = pipe.lib
    configs = [(fam, 32, 2048) for fam in ("uniform", "sparse", "tie", "noisy_linear", "metric", "low_rank",
                                           "clustered")]
    configs.append(("uniform", 1, 16384))
    lines = []
    for fam, B, n in configs:
        if n <= 4096:
            C = torch.from_numpy(np.stack([generate_family(fam, n, 100 + b) for b in range(B)])).to(dev)
        else:
            g = torch.Generator(device=dev).manual_seed(5)
            C = torch.rand((B, n, n), dtype=torch.float64, device=dev, generator=g)
        x, _, ret_jv, _ = pipe.lapjv_batch(C, want_stats=False)
        ms_jv, _ = timed(lambda: pipe.lapjv_batch(C, want_stats=False), max(1, args.reps // 2))
        out = {}

        def run():
            out["r"] = pipe.oracle_duals_batch(C, x)
        ms_od, ms_od_min = timed(run, args.reps)
        _, u, v, ret, sweeps = out["r"]
        sw = sweeps.cpu().numpy()
        colout = torch.empty((B, n), dtype=torch.float64, device=dev)
        nb = int(lib.lapwarm_sweep_workspace_bytes(B, n))
        ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def colmin():
            rc = lib.lapwarm_colmin_batched(C.data_ptr(), B, n, None, colout.data_ptr(), ws.data_ptr(), nb,
                                            ct.c_void_p(stream))
            assert rc == 0
        ms_cm, _ = timed(colmin, args.reps)
        rows_read = int(sw[:, 2].sum())
        line = dict(family=fam, batch=B, n=n, oracle_ms=round(ms_od, 3), oracle_ms_min=round(ms_od_min, 3),
                    lapjv_ms=round(ms_jv, 3), colmin_ms=round(ms_cm, 4),
                    ret_ok=int((ret == 0).sum()), lapjv_ok=int((ret_jv == 0).sum()),
                    sweeps_max=int(sw[:, 0].max()), sweeps_mean=round(float(sw[:, 0].mean()), 1),
                    depth_max=int(sw[:, 1].max()), replayed=int(sw[:, 3].sum()),
                    row_sets_read=round(rows_read / (B * n), 2),
                    sweep_GBps_lower=round(rows_read * n * 8 / (ms_od * 1e-3) / 1e9, 1),
                    colmin_GBps=round(B * n * n * 8 / (ms_cm * 1e-3) / 1e9, 1))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del C, x, out
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
