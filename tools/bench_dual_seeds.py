#!/usr/bin/env python3
"""Dual projection and classical seeds of a mixed-size batch on the MI355X: timings against the per-instance loop,
and the seed-sensitivity table of the seeded solver.

Timing, two cases, one JSON line each (NumPy in, NumPy out on both sides, as a user of `solvers` calls them):
  distinct  B instances of B distinct sizes spread evenly over [lo, hi] (uniform family)
  same      B instances of one size n, where only the saved read of C and the saved copies can help
`project_loop` / `project_many` are solvers.project_feasible per instance against one
solvers.project_feasible_many call, from infeasible seeds (uniform in [0, 1)); `seed_loop` / `seed_many` are
solvers.seed_row_col_minima per instance against solvers.seed_row_col_minima_many.  For the one-size case the
device-resident round is timed as well, through the C ABI on buffers made once: `round_uniform` is
lapwarm_project_round_batched on the stacked block (five kernels, three reads of C) and `round_ragged` is
lapwarm_project_feasible_ragged with max_rounds = 1 on the same block as a padded pack (four kernels, two reads).
`resident_loop` / `resident_ragged` are the projection with costs and seeds already on the device, which is how
the pipeline calls it: one lapwarm_project_round_batched per instance and round with the host reading gmin after
each (what lapwarm_project_feasible does) against WarmStartPipeline.project_feasible_ragged on a pack made once.
Each figure is a host-clock mean over `inner` back-to-back calls after `warmup` untimed ones, with one device
synchronise at the end; `reps` of them are listed, so that the run-to-run spread can be read beside the median.

Seed sensitivity, one JSON line per seed kind on the distinct batch: the seeded solver's `paths` and `finds`
counters (summed over the batch, from `stats`) and the branch each instance took after seeded_ragged from row/col minima, from the oracle duals,
and from the oracle duals plus N(0, s) noise re-projected (noisy_duals_ragged) at s = 0.01, 0.05, 0.15.

`--pkg DIR` times another checkout of the package with the same inputs; a checkout without the *_many functions
reports the loops and the uniform round only: that is how a baseline is taken in the same session.

Usage:  python tools/bench_dual_seeds.py [--batch 32] [--lo 384] [--hi 640] [--n 512] [--reps 3] [--inner 5]
                                         [--warmup 2] [--pkg DIR] [--out FILE]
"""
import argparse
import ctypes as ct
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
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pkg", default=str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd"))
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.pkg).resolve()))

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dual_seeds.py needs the MI355X: nothing here is measured on a CPU")
    import solvers
    from gnn import OneGNN, WarmStartPipeline
    from gnn.features import ragged_pack
    from lap import _hip
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pipe = WarmStartPipeline(OneGNN(21, 64, 2).eval(), dev)
    lib = _hip.require_device()
    label = args.label or Path(args.pkg).resolve().parent.name
    has_many = hasattr(solvers, "project_feasible_many")
    lines = []

    def times(fn, inner=args.inner):
        out = []
        for _ in range(args.reps):
            for _ in range(args.warmup):
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

    def inputs(sizes):
        rs = np.random.RandomState(len(sizes) * 1000 + sizes[0])
        costs = [rs.uniform(0.0, 1.0, (m, m)) for m in sizes]
        return costs, [rs.uniform(0.0, 1.0, m) for m in sizes], [rs.uniform(0.0, 1.0, m) for m in sizes]

    def run(case, sizes):
        costs, us, vs = inputs(sizes)
        line = dict(case=case, label=label, batch=len(sizes), sizes=[min(sizes), max(sizes)],
                    distinct_sizes=len(set(sizes)))

        def project_loop():
            return [solvers.project_feasible(C, u, v) for C, u, v in zip(costs, us, vs)]

        def seed_loop():
            return [solvers.seed_row_col_minima(C) for C in costs]

        ref_p, ref_s = project_loop(), seed_loop()
        line.update(stats("project_loop", times(project_loop)))
        line.update(stats("seed_loop", times(seed_loop)))
        if has_many:
            got_p = solvers.project_feasible_many(costs, us, vs, pipeline=pipe)
            got_s = solvers.seed_row_col_minima_many(costs, pipeline=pipe)
            line["bit_equal_to_loop"] = all(np.array_equal(a[k], b[k]) for got, ref in ((got_p, ref_p), (got_s, ref_s))
                                            for a, b in zip(got, ref) for k in (0, 1))
            line.update(stats("project_many", times(lambda: solvers.project_feasible_many(costs, us, vs,
                                                                                          pipeline=pipe))))
            line.update(stats("seed_many", times(lambda: solvers.seed_row_col_minima_many(costs, pipeline=pipe))))
            line["project_loop_over_many"] = round(line["project_loop_median_ms"] / line["project_many_median_ms"], 2)
            line["seed_loop_over_many"] = round(line["seed_loop_median_ms"] / line["seed_many_median_ms"], 2)
        # the same work with the costs and seeds resident on the device, which is how the pipeline calls it: the loop
        # is one lapwarm_project_round_batched per instance and round with the host reading gmin after each, as
        # lapwarm_project_feasible does it; the ragged side is project_feasible_ragged on a pack made once
        Cd = [torch.from_numpy(C).to(dev).unsqueeze(0) for C in costs]
        ud = [torch.from_numpy(u).to(dev) for u in us]
        vd = [torch.from_numpy(v).to(dev) for v in vs]
        g1 = torch.empty(1, dtype=torch.float64, device=dev)
        ws1 = {m: torch.empty(int(lib.lapwarm_sweep_workspace_bytes(1, m)), dtype=torch.uint8, device=dev)
               for m in set(sizes)}
        s0 = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def resident_loop():
            out = []
            for C, u, v in zip(Cd, ud, vd):
                u, v, m = u.clone(), v.clone(), C.shape[1]
                for _ in range(50):
                    rc = lib.lapwarm_project_round_batched(C.data_ptr(), 1, m, u.data_ptr(), v.data_ptr(),
                                                           g1.data_ptr(), ws1[m].data_ptr(), ws1[m].numel(), s0)
                    assert rc == 0, rc
                    if float(g1) >= -1e-12:
                        break
                out.append((u, v))
            return out

        line.update(stats("resident_loop", times(resident_loop)))
        if has_many:
            rpack = ragged_pack([C[0] for C in Cd], dev)
            up = torch.nn.utils.rnn.pad_sequence(ud, batch_first=True).contiguous()
            vp = torch.nn.utils.rnn.pad_sequence(vd, batch_first=True).contiguous()
            got = pipe.project_feasible_ragged(rpack, up, vp)
            line["resident_bit_equal_to_loop"] = all(
                torch.equal(got[0][b, :len(u)], u) and torch.equal(got[1][b, :len(v)], v)
                for b, (u, v) in enumerate(resident_loop()))
            line.update(stats("resident_ragged", times(lambda: pipe.project_feasible_ragged(rpack, up, vp))))
            line["resident_loop_over_ragged"] = round(line["resident_loop_median_ms"] /
                                                      line["resident_ragged_median_ms"], 2)
        if len(set(sizes)) == 1:  # the device-resident round, uniform against ragged, through the C ABI
            n, B = sizes[0], len(sizes)
            C = torch.from_numpy(np.stack(costs)).to(dev)
            u0, v0 = torch.from_numpy(np.stack(us)).to(dev), torch.from_numpy(np.stack(vs)).to(dev)
            u, v = u0.clone(), v0.clone()
            gmin = torch.empty(B, dtype=torch.float64, device=dev)
            nb = int(lib.lapwarm_sweep_workspace_bytes(B, n))
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            stream = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def round_uniform():
                rc = lib.lapwarm_project_round_batched(C.data_ptr(), B, n, u.data_ptr(), v.data_ptr(),
                                                       gmin.data_ptr(), ws.data_ptr(), nb, stream)
                assert rc == 0, rc

            line.update(stats("round_uniform", times(round_uniform, 20 * args.inner)))
            if has_many:
                pack = ragged_pack(C, dev, sizes=sizes)
                rounds = torch.empty(B, dtype=torch.int32, device=dev)
                ret = torch.empty(B, dtype=torch.int32, device=dev)
                nb2 = int(lib.lapwarm_ragged_duals_workspace_bytes(B, n))
                ws2 = torch.empty(nb2, dtype=torch.uint8, device=dev)

                def round_ragged():
                    rc = lib.lapwarm_project_feasible_ragged(
                        pack.C.data_ptr(), pack.offsets.data_ptr(), pack.sizes.data_ptr(), pack.ld, B, n,
                        u.data_ptr(), v.data_ptr(), 1, 1e-12, gmin.data_ptr(), rounds.data_ptr(), ret.data_ptr(),
                        ws2.data_ptr(), nb2, stream)
                    assert rc == 0, rc

                line.update(stats("round_ragged", times(round_ragged, 20 * args.inner)))
                line["round_uniform_over_ragged"] = round(line["round_uniform_median_ms"] /
                                                          line["round_ragged_median_ms"], 2)
        emit(line)
        return costs

    B = args.batch
    distinct = [int(x) for x in np.linspace(args.lo, args.hi, B).round()]
    costs = run("distinct", distinct)
    run("same", [args.n] * B)

    if has_many:  # the seed-sensitivity table on the distinct batch
        from gnn.pipeline import STATS_FIELDS
        pack = ragged_pack(costs, dev)
        duals = pipe.oracle_duals_many(costs)
        assert int(duals.ret.abs().sum()) == 0
        kinds = [("row_col_minima", pipe.seed_row_col_minima_ragged(pack)[:2]), ("oracle", (duals.u, duals.v))]
        for s in (0.01, 0.05, 0.15):
            g = torch.Generator(device=dev)
            g.manual_seed(0)
            kinds.append((f"oracle_noise_{s}", pipe.noisy_duals_ragged(pack, duals.u, duals.v, s, generator=g)[:2]))
        for name, (u, v) in kinds:
            x, _, ret, st = pipe.seeded_ragged(pack, u.contiguous(), v.contiguous())
            torch.cuda.synchronize()
            emit(dict(case="seed_sensitivity", label=label, seed=name, batch=B, sizes=[min(distinct), max(distinct)],
                      ret_nonzero=int((ret != 0).sum()), same_matching_as_oracle=bool(torch.equal(x, duals.x.to(x.dtype))),
                      branches={str(k): int(c) for k, c in zip(*np.unique(
                          st[:, STATS_FIELDS.index("branch")].cpu().numpy(), return_counts=True))},
                      paths=int(st[:, STATS_FIELDS.index("paths")].sum()),
                      finds=int(st[:, STATS_FIELDS.index("finds")].sum())))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
