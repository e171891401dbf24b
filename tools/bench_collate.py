#!/usr/bin/env python3
"""Time the ragged front end (gnn.features.row_features_ragged, gnn.collate_device) on the MI355X.

Two cases, one JSON line each:
  equal  B x n x n fp64 resident on the device, all instances of one size: the ragged call with cost32
         (padded form, ld = n) against row_features_device followed by C.to(float32), which is what a caller
         had before.  `ragged_kernels_ms` leaves out the upload of offsets and sizes (the batch packed once).
  mixed  B host matrices with sizes spread evenly over [lo, hi]: collate_device against the reference's
         `collate` done with this package's own per-instance entry: compute_row_features per instance, a
         zero-padded float32 batch filled on the host, then moved to the device.
Both sides are timed with a host clock around work that ends in a device synchronise, alternating, after a
warm-up of each; the device-resident figures are means over back-to-back calls.

Usage:  python tools/bench_collate.py [--batch 32] [--n 2048] [--lo 512] [--hi 2048] [--reps 5] [--out FILE]
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


def mean_ms(fn, inner):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_collate(items, device):
    """`collate` of gnn/train_one_gnn.py:72-91 with compute_row_features per instance, then to the device."""
    from gnn import ROW_FEATURE_DIM, compute_row_features
    B, N = len(items), max(it["n"] for it in items)
    cost = torch.zeros(B, N, N, dtype=torch.float32)
    u = torch.zeros(B, N, dtype=torch.float32)
    v = torch.zeros(B, N, dtype=torch.float32)
    feat = torch.zeros(B, N, ROW_FEATURE_DIM, dtype=torch.float32)
    mask = torch.zeros(B, N, dtype=torch.bool)
    for b, it in enumerate(items):
        n = it["n"]
        cost[b, :n, :n] = torch.from_numpy(it["cost"].astype(np.float32, copy=False))
        u[b, :n] = torch.from_numpy(it["u"].astype(np.float32, copy=False))
        v[b, :n] = torch.from_numpy(it["v"].astype(np.float32, copy=False))
        feat[b, :n] = torch.from_numpy(compute_row_features(it["cost"]))
        mask[b, :n] = True
    return tuple(t.to(device) for t in (cost, u, v, feat, mask))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--lo", type=int, default=512)
    ap.add_argument("--hi", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_collate.py needs the MI355X: nothing here is measured on a CPU")
    from gnn import collate_device
    from gnn.features import ragged_pack, row_features_device, row_features_packed, row_features_ragged
    dev = torch.device("cuda:0")
    lines = []

    B, n = args.batch, args.n
    g = torch.Generator(device=dev).manual_seed(n)
    C = torch.rand((B, n, n), dtype=torch.float64, device=dev, generator=g)
    sizes = [n] * B
    pack = ragged_pack(C, sizes=sizes)

    def uniform():
        feat, topk = row_features_device(C)
        return feat, topk, C.to(torch.float32)

    def ragged():
        return row_features_ragged(C, want_cost32=True, sizes=sizes)

    def ragged_kernels():
        return row_features_packed(pack, want_cost32=True)

    t_uni, t_rag, t_ker = [], [], []
    for _ in range(args.reps):
        t_uni.append(mean_ms(uniform, args.inner))
        t_rag.append(mean_ms(ragged, args.inner))
        t_ker.append(mean_ms(ragged_kernels, args.inner))
    f0, k0, c0 = uniform()
    r = ragged()
    line = dict(case="equal", batch=B, n=n, uniform_plus_cast_ms=round(float(np.median(t_uni)), 4),
                ragged_ms=round(float(np.median(t_rag)), 4), ragged_kernels_ms=round(float(np.median(t_ker)), 4),
                ratio_uniform_over_ragged=round(float(np.median(t_uni) / np.median(t_rag)), 3),
                same_bits=bool(torch.equal(f0, r.feat) and torch.equal(k0, r.topk) and torch.equal(c0, r.cost32)))
    print(json.dumps(line), flush=True)
    lines.append(line)
    del C, pack, f0, k0, c0, r

    rs = np.random.RandomState(0)
    mixed = [int(x) for x in np.linspace(args.lo, args.hi, B).round()]
    items = [{"cost": rs.uniform(0.0, 1.0, (m, m)), "u": rs.normal(0.0, 0.1, m), "v": rs.normal(0.0, 0.1, m), "n": m}
             for m in mixed]
    timed(lambda: collate_device(items, dev))
    timed(lambda: host_collate(items, dev))
    t_dev, t_host = [], []
    for _ in range(args.reps):
        ms, bt = timed(lambda: collate_device(items, dev))
        t_dev.append(ms)
        ms, ref = timed(lambda: host_collate(items, dev))
        t_host.append(ms)
    pack = ragged_pack([it["cost"] for it in items], dev)
    ker = mean_ms(lambda: row_features_packed(pack, want_cost32=True), args.inner)
    line = dict(case="mixed", batch=B, sizes=[mixed[0], mixed[-1]], collate_device_ms=round(float(np.median(t_dev)), 2),
                host_collate_ms=round(float(np.median(t_host)), 2), ragged_kernels_ms=round(ker, 4),
                speedup=round(float(np.median(t_host) / np.median(t_dev)), 2),
                same_bits=bool(torch.equal(bt.cost, ref[0]) and torch.equal(bt.row_feat, ref[3])
                               and torch.equal(bt.mask, ref[4]) and torch.equal(bt.u, ref[1])))
    print(json.dumps(line), flush=True)
    lines.append(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
