"""Times the pruned exact solve (WarmStartPipeline.lapjv_pruned_ragged) against the dense cold solve on resident
cost matrices: alternating runs, `--reps` of each, every value listed, one JSON line per case.

    python tools/bench_pruned.py [--reps 3] [--cases k3,mixed,uniform,sweep,lowrank,single] [--ks 8,16,32]
                                 [--big 4096,8192] [--sweep 768,1024,1536] [--out FILE]

Cases (32 instances each unless single):
  k3        32 x 2048 of the K3 family mix (solvers.generators.mixed_batch)
  mixed     32 distinct sizes over 384..640, the four K3 families cycled over the instances
  uniform   the same sizes, uniform costs only
  sweep     32 x n uniform costs for every n of --sweep: where the pruned route stops winning
  lowrank   32 x 512 of the low_rank family
  single    one uniform instance per n of --big
k over --ks; without a seed and with the column minima (the min-trick of u = 0) as seed.  Two dense baselines:
`dense` is lapjv_batch, one call per distinct size; `dense_ragged` sends the sizes lapjv_ragged takes (n <= 511)
through one ragged call and the rest through lapjv_batch.  For every case one more line times solve_pruned_many
(model seed, dense fallback) against solve_many (the seeded dense route) with the tool's untrained OneGNN, and one
times the grow steps: round 0 and one pricing step from the first solve's duals, against torch.sum over the same
bytes (a plain read).  Wall time around a device synchronisation: the pruned loop reads a few words back per round,
so its host time is part of what a caller pays."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd")]

K3_FAMILIES = ("uniform", "sparse", "metric", "clustered")


def timed(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="k3,mixed,uniform,sweep,lowrank,single")
    ap.add_argument("--big", default="4096,8192")
    ap.add_argument("--sweep", default="768,1024,1536")
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from gnn import OneGNN, WarmStartPipeline
    from gnn.features import RaggedPack, min_trick_ragged, ragged_pack
    from gnn.pipeline import SparsePack
    from solvers.generators import generate_family, mixed_batch

    torch.manual_seed(0)
    pipe = WarmStartPipeline(OneGNN(21, 64, 2).eval(), "cuda:0")
    dev = pipe.device
    sink = open(args.out, "w") if args.out else None
    which = args.cases.split(",")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    sizes32 = [int(n) for n in np.random.default_rng(5).choice(np.arange(384, 641), size=32, replace=False)]
    cases = []  # (name, matrices, families)
    if "k3" in which:
        C, fams = mixed_batch(32, 2048, seed=3)
        cases.append(("k3_32x2048", [C[b] for b in range(32)], fams))
    if "mixed" in which:
        fams = [K3_FAMILIES[b % 4] for b in range(32)]
        cases.append(("mixed_384_640_k3mix", [generate_family(f, n, 1000 + n) for f, n in zip(fams, sizes32)], fams))
    if "uniform" in which:
        cases.append(("mixed_384_640_uniform", [generate_family("uniform", n, n) for n in sizes32], ["uniform"] * 32))
    if "sweep" in which:
        for n in (int(s) for s in args.sweep.split(",") if s):
            cases.append((f"uniform_32x{n}", [generate_family("uniform", n, 7 * n + b) for b in range(32)],
                          ["uniform"] * 32))
    if "lowrank" in which:
        cases.append(("lowrank_32x512", [generate_family("low_rank", 512, 50 + b) for b in range(32)],
                      ["low_rank"] * 32))
    if "single" in which:
        for n in (int(s) for s in args.big.split(",") if s):
            cases.append((f"single_{n}", [np.random.default_rng(n).random((n, n))], ["uniform"]))

    for name, mats, fams in cases:
        pack = ragged_pack(mats, dev)
        sizes = pack.host_sizes
        B = len(sizes)
        groups = {}
        for b, n in enumerate(sizes):
            groups.setdefault(n, []).append(b)
        dense_in = {n: torch.stack([torch.from_numpy(mats[b]) for b in g]).to(dev) for n, g in groups.items()}

        def dense():
            return {n: pipe.lapjv_batch(C, want_stats=False) for n, C in dense_in.items()}

        small = [b for b, n in enumerate(sizes) if pipe.lapjv_ragged_eligible(n)]
        sub = None
        if small:
            idx = torch.tensor(small, device=dev)
            hs = [sizes[b] for b in small]
            sub = RaggedPack(pack.C, pack.offsets[idx], pack.sizes[idx], None, None, pack.ld, max(hs), hs)

        def dense_ragged():
            out = [pipe.lapjv_ragged(sub, want_stats=False)] if sub is not None else []
            return out + [pipe.lapjv_batch(C, want_stats=False) for n, C in dense_in.items()
                          if not pipe.lapjv_ragged_eligible(n)]

        colmin = min_trick_ragged(pack, None)
        dres = dense()  # warm-up: workspaces and code objects
        dense_ragged()
        dense_cost = np.empty(B)
        for n, g in groups.items():
            xd = dres[n][0].cpu().numpy()
            for q, b in enumerate(g):
                dense_cost[b] = mats[b][np.arange(n), xd[q]].sum()
        for k in (int(s) for s in args.ks.split(",")):
            for seeded in (False, True):
                seed = colmin if seeded else None
                run = lambda: pipe.lapjv_pruned_ragged(pack, k, seed=seed)  # noqa: E731
                run()
                tp, td, tr, out = [], [], [], None
                for _ in range(args.reps):
                    ms, out = timed(run, torch)
                    tp.append(ms)
                    td.append(timed(dense, torch)[0])
                    tr.append(timed(dense_ragged, torch)[0])
                ret = out["ret"].cpu().numpy()
                nnz = out["nnz"].cpu().numpy().astype(np.float64)
                cost = out["cost"].cpu().numpy()
                ok = ret == 0
                n2 = np.asarray(sizes, dtype=np.float64) ** 2
                emit(dict(case=name, k=k, seed="colmin" if seeded else "none", pruned_ms=sorted(tp),
                          dense_ms=sorted(td), dense_ragged_ms=sorted(tr), ragged_instances=len(small),
                          rounds_max=int(out["rounds"].max()), rounds_mean=float(out["rounds"].float().mean()),
                          nnz_over_n2=float(np.mean(nnz[ok] / n2[ok])) if ok.any() else None,
                          refused_share=float(np.mean(ret == 3)), uncertified_share=float(np.mean(ret == 2)),
                          refused_families=sorted({fams[b] for b in range(B) if ret[b] == 3}),
                          max_rel_cost_diff=float(np.max(np.abs(cost[ok] - dense_cost[ok])
                                                         / np.maximum(1.0, np.abs(dense_cost[ok])))) if ok.any()
                          else None))

        # the two whole routes a caller has: model seed and dense fallback against the seeded dense solve
        costs_d = [pack.C[o:o + n * n].view(n, n) for o, n in zip(pack.offsets.tolist(), sizes)]
        pruned_many = lambda: pipe.solve_pruned_many(costs_d, k=16, use_model=True)  # noqa: E731
        seeded_many = lambda: pipe.solve_many(costs_d, want_stats=False)  # noqa: E731
        res = pruned_many()
        seeded_many()
        tp, ts = [], []
        for _ in range(args.reps):
            tp.append(timed(pruned_many, torch)[0])
            ts.append(timed(seeded_many, torch)[0])
        emit(dict(case=name, what="solve_pruned_many_k16_vs_solve_many", pruned_many_ms=sorted(tp),
                  solve_many_ms=sorted(ts), fallback_share=float(np.mean([r["fallback"] for r in res])),
                  rounds_max=max(r["rounds"] for r in res),
                  max_rel_cost_diff=float(max(abs(float(r["cost"]) - c) / max(1.0, abs(c))
                                              for r, c in zip(res, dense_cost)))))

        # the grow steps against a plain read of the same bytes: round 0, and a pricing step from the first solve
        csr, counts = pipe.prune_grow(pack, 16)
        added, _, gret = pipe.prune_counts(counts, B)
        live = [b for b in range(B) if gret[b] == 0]
        idx = torch.tensor(live, device=dev)
        hs = [sizes[b] for b in live]
        lp = RaggedPack(pack.C, pack.offsets[idx], pack.sizes[idx], None, None, pack.ld, max(hs), hs)
        lcsr = SparsePack(csr.cc, csr.kk, csr.ii, csr.nnz_offsets[idx], csr.row_offsets[idx], lp.sizes, hs,
                          [added[b] for b in live])
        sol, solve_ms = None, []
        for _ in range(2):
            ms, sol = timed(lambda: pipe.lapmod_ragged(lcsr, 3, want_stats=False), torch)
            solve_ms.append(ms)
        grow0 = lambda: pipe.prune_grow(pack, 16)  # noqa: E731
        price = lambda: pipe.prune_grow(lp, 16, key=sol["v"], x=sol["x"], csr=lcsr)  # noqa: E731
        read = lambda: pack.C.sum()  # noqa: E731
        grow0(), price(), read()
        tg, tq, tr = [], [], []
        for _ in range(max(args.reps, 5)):
            tg.append(timed(grow0, torch)[0])
            tq.append(timed(price, torch)[0])
            tr.append(timed(read, torch)[0])
        emit(dict(case=name, what="grow_k16_vs_read", grow_round0_ms=sorted(tg), grow_pricing_ms=sorted(tq),
                  read_ms=sorted(tr), first_lapmod_ms=sorted(solve_ms), live_instances=len(live),
                  bytes=int(pack.C.numel() * 8)))
        del pack, dense_in, csr, lcsr, sol, costs_d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
