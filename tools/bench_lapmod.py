"""Sparse LAPMOD against densify-and-solve on one MI355X: writes profiles/lapmod.jsonl and profiles/lapmod.md.

    python tools/bench_lapmod.py [--out-dir profiles] [--runs 3] [--calls N] [--cases a,b,c]

Cases: (a) 256 instances n = 128, k = 8 (tracker-like); (b) 32 instances n = 2048, k = 16; (c) one instance
n = 16384, k = 16.  Costs are integers 1..100, so augmentation runs.  Per case: `lap.lapmod_many` (checks, packing
and upload included), `WarmStartPipeline.lapmod_ragged` on a resident SparsePack, and `lapjv_batch` on the resident
densified matrices (absent = 1e5): what a user can do without the sparse solver.  Host clock around a window of
back-to-back calls (at least 0.3 s of work) after untimed ones, one device synchronise at the end; every run times
the three entries one after the other, so the sparse and the dense call alternate; the median of `runs` runs and
the spread (max - min) are reported.  The sparse and the dense cost are compared first."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd"))

# B, n, k, calls per timed window of the resident entries, of lapmod_many, title: every window is >= 0.3 s
CASES = {"a": (256, 128, 8, 400, 20, "256 instances, n = 128, k = 8 (tracker-like)"),
         "b": (32, 2048, 16, 10, 5, "32 instances, n = 2048, k = 16"),
         "c": (1, 16384, 16, 2, 2, "1 instance, n = 16384, k = 16")}


def make_problem(rng, n, k):
    """k random columns per row and a hidden permutation, costs 1..100, as (n, cc, ii, kk)."""
    perm = rng.permutation(n)
    cols = np.sort(np.concatenate([rng.integers(0, n, size=(n, k)), perm[:, None]], axis=1), axis=1)
    keep = np.concatenate([np.ones((n, 1), dtype=bool), np.diff(cols, axis=1) > 0], axis=1)
    ii = np.zeros(n + 1, dtype=np.int32)
    ii[1:] = np.cumsum(keep.sum(axis=1))
    kk = cols[keep].astype(np.int32)
    cc = rng.integers(1, 101, size=kk.size).astype(np.float64)
    return n, cc, ii, kk


def timed_alternating(fns, runs, sync):
    """fns: name -> (callable, calls).  Every run times each entry once, one after the other, so that the entries
    that are compared alternate inside one session; returns name -> (median ms per call, max - min)."""
    for fn, _ in fns.values():
        fn()
    sync()
    out = {name: [] for name in fns}
    for _ in range(runs):
        for name, (fn, calls) in fns.items():
            t = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            out[name].append((time.perf_counter() - t) / calls * 1e3)
    return {name: (statistics.median(v), max(v) - min(v)) for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=str(ROOT / "profiles"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="calls per run (0: the case's default)")
    ap.add_argument("--cases", default="a,b,c")
    args = ap.parse_args()
    import torch
    import lap
    from gnn.pipeline import shared_pipeline, sparse_pack
    pipe = shared_pipeline()
    dev = pipe.device
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    rng = np.random.default_rng(11)
    records = []
    for key in args.cases.split(","):
        B, n, k, calls, calls_many, title = CASES[key]
        calls = args.calls or calls
        probs = [make_problem(rng, n, k) for _ in range(B)]
        pack = sparse_pack(probs, dev)
        dense = torch.full((B, n, n), 1e5, dtype=torch.float64, device=dev)
        for b, (_, cc, ii, kk) in enumerate(probs):
            rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(ii))).to(dev)
            dense[b, rows, torch.from_numpy(kk.astype(np.int64)).to(dev)] = torch.from_numpy(cc).to(dev)
        res = pipe.lapmod_ragged(pack, 3)
        xd = pipe.lapjv_batch(dense, want_stats=False)[0]
        sync()
        ok = bool((res["ret"] == 0).all())
        sparse_cost = [lap.get_cost(*probs[b], res["x"][b, :n].cpu().numpy()) for b in range(min(B, 8))]
        dense_cost = [float(dense[b, torch.arange(n, device=dev), xd[b].long()].sum()) for b in range(min(B, 8))]
        stats = res["stats"].cpu().numpy()
        rec = {"case": key, "title": title, "B": B, "n": n, "k": k, "calls": calls, "runs": args.runs,
               "all_solved": ok, "same_cost": sparse_cost == dense_cost,
               "paths_mean": float(stats[:, 4].mean()), "arr_iters_mean": float(stats[:, 3].mean()),
               "search": int(stats[0, 11])}
        times = timed_alternating({
            "lapmod_ragged": (lambda: pipe.lapmod_ragged(pack, 3, want_stats=False), calls),
            "lapjv_batch_dense": (lambda: pipe.lapjv_batch(dense, want_stats=False), calls),
            "lapmod_many": (lambda: lap.lapmod_many(probs), calls_many)}, args.runs, sync)
        rec["calls_many"] = calls_many
        for name, (ms, spread) in times.items():
            rec[name + "_ms"], rec[name + "_spread_ms"] = ms, spread
        records.append(rec)
        print(json.dumps(rec), flush=True)
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    with open(out / "lapmod.jsonl", "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    lines = ["# Sparse LAPMOD against densify-and-solve: what was measured", "",
             "One MI355X, `tools/bench_lapmod.py` (`profiles/lapmod.jsonl`): host-clock mean per call over a window of",
             "back-to-back calls (400 / 10 / 2 calls at (a) / (b) / (c); `lapmod_many` 20 / 5 / 2) after an untimed one,",
             "one device synchronise at the end; every run times the entries one after the other, so the sparse and the",
             "dense call alternate; the median of the runs with the run-to-run spread (max - min).",
             "Costs are integers 1..100; FP_DYNAMIC.  `lapjv_batch` solves the densified matrices",
             "(absent = 1e5), resident on the device.", "",
             "| case | lapmod_many (from NumPy) | lapmod_ragged (resident) | lapjv_batch, densified | dense / ragged |",
             "|---|---|---|---|---|"]
    for r in records:
        ratio = r["lapjv_batch_dense_ms"] / r["lapmod_ragged_ms"]
        lines.append("| (%s) %s | %.3f ms (spread %.3f) | %.3f ms (%.3f) | %.3f ms (%.3f) | %.2f x (%s) |" % (
            r["case"], r["title"], r["lapmod_many_ms"], r["lapmod_many_spread_ms"], r["lapmod_ragged_ms"],
            r["lapmod_ragged_spread_ms"], r["lapjv_batch_dense_ms"], r["lapjv_batch_dense_spread_ms"], ratio,
            "sparse faster" if ratio > 1 else "sparse slower"))
    lines += ["", "Per case, mean over instances: " + "; ".join(
        "(%s) %.0f ARR iterations, %.1f paths, search %d, all solved %s, same cost as dense %s" % (
            r["case"], r["arr_iters_mean"], r["paths_mean"], r["search"], r["all_solved"], r["same_cost"])
        for r in records) + "."]
    (out / "lapmod.md").write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
