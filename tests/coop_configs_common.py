"""The cooperative-kernel configurations the suite runs: one row per way of reaching an instantiation of
coop_ssp_kernel<CH, NL> (csrc/coop_ssp.hip, kCoopKernels) through the planner's rules (csrc/solve_plan.hip,
coop_config) and the environment switches, the sweeps under switches that change cooperative or helper code
paths, and the helpers the tests of these rows share.  test_host_logic.py checks on the CPU that the planner
plans what the rows say; test_gpu_coop_instantiations.py runs them.

The planner's rules: members = ceil(n / (64 CH)); NL = (4 members + 24 + 63) // 64 -- 1 up to 10 members, 2 for
11 .. 26, 3 for 27 .. 32; CH by size is 1 up to n = 512, 2 up to 1024, 4 up to 8192, 8 above, or LAPWARM_COOP_CH.
The switches are read once per process, so every row with an environment runs in a child process.

As a command (`python coop_configs_common.py n ...`) this prints, as JSON, lapwarm_coop_members(n) and every
field of the seeded plan of one instance for each n, in the environment it runs in."""
import json
import sys
from collections import namedtuple
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd"
DRIVER = ROOT / "tests" / "native" / "_build" / "parity_driver"

# the instantiations csrc/coop_ssp.hip ships (kCoopKernels), written out: one added there needs a row here
COOP_KERNELS = {(1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2), (4, 3), (8, 1), (8, 2), (8, 3), (16, 1), (16, 2)}

MIN_N = {"LAPWARM_COOP_MIN_N": "1"}  # the cooperative chain from n = 1 on (default: 4428)


def _forced(ch):
    return dict(MIN_N, LAPWARM_COOP_CH=str(ch))


# where a row runs: "sweep" = the native driver's ten families x seed kinds + nine cold solves at that one size
# (58 cases), "single" = one seeded_batch call against the oracle (too large for the sweep), "parity" = an
# existing test of test_gpu_parity.py (listed so that the rows cover every instantiation)
CoopConfig = namedtuple("CoopConfig", "label env n members kernel runs timeout")

# timeout: seconds the child process may take: five times the wall time of its first run on an MI355X (the
# column `measured`: seconds from the child's start to its exit, reps = 1, the oracle's CPU solves included),
# at least 30 s -- process start-up and the first GPU call do not shrink with n.  Five sweeps take longer than
# 20 s (c1_26, c4_10, c4_11, c8_5, c16_3, as do the helper sweeps): 58 solves on either side at n >= 1664 (the
# one-workgroup kernel's sweep is no quicker: helpers_4 spends 29 of its 41 s on n = 2048).  The tie-heavy families are the point of the rows, so none is thinned.
CONFIGS = (
    #          label      env          n      members <CH,NL>  runs      timeout   measured  what it is for
    CoopConfig("c1_12",   _forced(1),  705,   12,     (1, 2),  "sweep",  30),   #   3.5   first NL = 2 class (11 .. 16); last member 1 position
    CoopConfig("c1_17",   _forced(1),  1025,  17,     (1, 2),  "sweep",  40),   #   7.5   first size whose records exceed one register; last member 1 position
    CoopConfig("c1_26",   _forced(1),  1664,  26,     (1, 2),  "sweep",  110),  #  21.5   largest two-load poll, all members full
    CoopConfig("c2_8",    MIN_N,       777,   7,      (2, 1),  "sweep",  30),   #   4.5   full sweep at CH = 2; last member partly empty (9 of 128)
    CoopConfig("c2_12",   _forced(2),  1409,  12,     (2, 2),  "sweep",  80),   #  16.1   last member 1 position
    CoopConfig("c4_5",    MIN_N,       1025,  5,      (4, 1),  "sweep",  40),   #   7.8   last member 1 position
    CoopConfig("c4_10",   MIN_N,       2560,  10,     (4, 1),  "sweep",  360),  #  72.1   largest one-load poll, all members full
    CoopConfig("c4_11",   MIN_N,       2561,  11,     (4, 2),  "sweep",  360),  #  72.8   first two-load poll; last member 1 position; tie families
    CoopConfig("c8_2",    _forced(8),  513,   2,      (8, 1),  "sweep",  30),   #   2.6   two members, the second 1 position
    CoopConfig("c8_5",    _forced(8),  2049,  5,      (8, 1),  "sweep",  220),  #  44.0   last member 1 position
    CoopConfig("c16_2",   _forced(16), 1025,  2,      (16, 1), "sweep",  60),   #  11.8   16 positions per lane, last member 1 position
    CoopConfig("c16_3",   _forced(16), 2050,  3,      (16, 1), "sweep",  270),  #  53.1   even n (16-byte row prefetch on), last member 2 positions
    CoopConfig("c16_11",  _forced(16), 10241, 11,     (16, 2), "single", 300),  #  59.8   the only class that reaches <16, 2>; last member 1 position (11.0 s before its tie instance)
    CoopConfig("c4_27",   {},          6657,  27,     (4, 3),  "single", None),  # 12.1   first three-load poll; odd n; last member 1 position (in process)
    CoopConfig("k1_8",    MIN_N,       512,   8,      (1, 1),  "parity", None),  #        test_cooperative_kernel_forced_on_small_sizes_native_sweep (n = 1 .. 512)
    CoopConfig("k8_18",   {},          9216,  18,     (8, 2),  "parity", None),  #        test_cooperative_kernel_member_counts[9216]
    CoopConfig("k8_32",   {},          16384, 32,     (8, 3),  "parity", None),  #        test_large_n_pipeline_exact[16384]
)

# Sweeps under the switches no other test sets.  plan: what the seeded plan of one instance must say at every
# size (field of plan_fields() -> value), so that a switch the library ignores cannot pass as tested.
# timeout and `measured` as above.
SwitchSweep = namedtuple("SwitchSweep", "label env sizes members plan timeout")

SWITCH_SWEEPS = (
    # mailbox stores stay agent-scope: one-member, few-member and CH = 2 exchanges (measured 6.9)
    SwitchSweep("xcd_stores_0", dict(MIN_N, LAPWARM_COOP_XCD_STORES="0"), (64, 200, 512, 777), (1, 4, 8, 7),
                {"coop_xcd_stores": 0}, 35),
    # one cooperative launch: phase 2 finishes every path left after the first bail (measured 5.7)
    SwitchSweep("relaunches_0", dict(MIN_N, LAPWARM_COOP_RELAUNCHES="0"), (200, 512, 777), (4, 8, 7),
                {"coop_pairs": 0}, 30),
    # exactly one hand-over to phase 3 and back, then phase 2 (measured 5.8)
    SwitchSweep("relaunches_1", dict(MIN_N, LAPWARM_COOP_RELAUNCHES="1"), (200, 512, 777), (4, 8, 7),
                {"coop_pairs": 1}, 30),
    # several helper workgroups per instance, at the even sizes that get them (measured 41.4 and 42.4)
    SwitchSweep("helpers_4", {"LAPWARM_HELPERS_PER_INSTANCE": "4"}, (1024, 1026, 2048), (0, 0, 0), {"helper": 4}, 210),
    SwitchSweep("helpers_2", {"LAPWARM_HELPERS_PER_INSTANCE": "2"}, (1024, 1026, 2048), (0, 0, 0), {"helper": 2}, 210),
)

CASES_PER_SIZE = 58  # of a driver sweep with reps = 1: 49 seeded (family, seed kind) pairs + 9 cold solves

# lapwarm::plan_solve's fields in declaration order (solve_plan_common.plan_solve flattens them)
PLAN_FIELDS = ("shape",
               "prep_threads", "prep_ch", "prep_ldsl", "prep_tb", "prep_lists", "prep_lds_bytes",
               "paths_threads", "paths_ch", "paths_ldsl", "paths_tb", "paths_lists", "paths_lds_bytes",
               "helper",
               "coop_ch", "coop_nl", "coop_members", "coop_mail_granules", "coop_per_launch", "coop_pairs",
               "coop_xcd_stores")


def plan_fields(lib, n):
    """Seeded plan of ONE instance (what the driver's host API solves per call) on a 256-CU device."""
    import solve_plan_common as spc
    return dict(zip(PLAN_FIELDS, spc.plan_solve(lib)(spc.MODES[0], 1, n, 0, False, 256)))


def planned(env, sizes, timeout=600):
    """-> [(lapwarm_coop_members(n), plan fields)] per size, from a fresh interpreter with `env` set."""
    import os
    import subprocess
    r = subprocess.run([sys.executable, __file__] + [str(n) for n in sizes], capture_output=True, text=True,
                       timeout=timeout, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-2000:]
    return [(m, p) for m, p in json.loads(r.stdout)]


def run_sweep(env, sizes, timeout):
    """The native driver at exactly `sizes` (PARITY_SIZES), reps = 1, in a child process under its own time
    limit.  -> ({n: coop_members of its progress line}, seconds).  Asserts exit status 0, bad=0 and that no
    family, seed kind or cold solve went missing.  Never retried: a time-out or a signal is a finding."""
    import os
    import re
    import subprocess
    import time
    assert DRIVER.exists(), "build it with __graft_entry__.build()"
    t0 = time.monotonic()
    proc = subprocess.run([str(DRIVER), "0", "1"], capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, PARITY_SIZES=",".join(str(n) for n in sizes), **env))
    secs = time.monotonic() - t0
    print(f"sweep {sizes} {env}: {secs:.1f} s\n{proc.stdout[-1500:]}")
    assert proc.returncode == 0, (proc.returncode, proc.stdout[-3000:], proc.stderr[-1000:])
    summary = proc.stdout.splitlines()[-1]
    assert summary.startswith("SUMMARY ") and " bad=0 " in summary, summary
    assert f" total={CASES_PER_SIZE * len(sizes)} " in summary, summary
    seen = {int(n): int(m) for n, m in re.findall(r"^\[n<=(\d+)\] cases=\d+ bad=0 elapsed=\S+ coop_members=(\d+)$",
                                                   proc.stdout, re.M)}
    assert sorted(seen) == sorted(sizes), (seen, proc.stdout[-1500:])
    return seen, secs


def rowmin32_seeds(C):
    """The driver's `rowmin32` recipe: row minima rounded through float32, v from the min-trick in float32
    arithmetic on float32-rounded costs.  Such seeds make collections tie; the cooperative kernel handles a
    single tie itself and hands the path to jv_instance_kernel when there are several."""
    import numpy as np
    n = C.shape[0]
    u32 = C.min(axis=1).astype(np.float32)
    v32 = np.full(n, np.inf, dtype=np.float32)
    for lo in range(0, n, 1024):  # (row blocks: no n x n temporary)
        v32 = np.minimum(v32, (C[lo:lo + 1024].astype(np.float32) - u32[lo:lo + 1024, None]).min(axis=0))
    return u32.astype(np.float64), v32.astype(np.float64)


def rowmin_seeds(C):
    """Row minima and the fp64 min-trick."""
    import numpy as np
    u = C.min(axis=1)
    v = np.full(C.shape[0], np.inf)
    for lo in range(0, C.shape[0], 1024):
        v = np.minimum(v, (C[lo:lo + 1024] - u[lo:lo + 1024, None]).min(axis=0))
    return u, v


def single_case_inputs(label):
    """-> (Cs, us, vs, names) of a "single" row."""
    import numpy as np
    from solvers.generators import mixed_batch
    n = {c.label: c.n for c in CONFIGS}[label]
    Cs = [np.random.RandomState(23).uniform(0, 1, (n, n))]
    seeds = [rowmin32_seeds(Cs[0])]
    names = ["uniform/rowmin32"]
    if label == "c4_27":
        Cs.append(mixed_batch(1, n, families=("sparse",), seed=29)[0][0])
        seeds.append(rowmin_seeds(Cs[1]))
        names.append("sparse/rowmin")
    else:
        assert label == "c16_11", label
    # The instances above end every path inside the cooperative kernel (measured: no path handed to phase 3,
    # float32-rounded seeds or not).  Tie-family costs with row-min seeds give collections with several ties,
    # where the kernel stops and jv_instance_kernel searches the path: the hand-over at this (CH, NL), measured
    # 96 times per instance -- every (cooperative, phase 3) pair of the chain -- before phase 2 finishes the rest.
    Cs.append(mixed_batch(1, n, families=("tie",), seed=31)[0][0])
    seeds.append(rowmin_seeds(Cs[-1]))
    names.append("tie/rowmin")
    return np.stack(Cs), np.stack([s[0] for s in seeds]), np.stack([s[1] for s in seeds]), names


def run_single_case(label):
    """One seeded_batch call of a "single" row against oracle.jv.seeded_raw: the planner chose the row's
    geometry, the cooperative kernel took part, x / y / ret bit-equal, path / collection / relax-step /
    element counters equal."""
    import numpy as np
    import torch
    from gnn import OneGNN, WarmStartPipeline
    from lap import _hip
    from oracle import jv
    cfg = {c.label: c for c in CONFIGS}[label]
    lib = _hip.load()
    plan = plan_fields(lib, cfg.n)
    assert lib.lapwarm_coop_members(cfg.n) == cfg.members, lib.lapwarm_coop_members(cfg.n)
    assert (plan["coop_ch"], plan["coop_nl"]) == cfg.kernel, plan
    Cs, us, vs, names = single_case_inputs(label)
    pipe = WarmStartPipeline(OneGNN(21, hidden=64, layers=2).eval(), "cuda:0")
    x, y, ret, stats = pipe.seeded_batch(torch.from_numpy(Cs).cuda(), torch.from_numpy(us).cuda(),
                                         torch.from_numpy(vs).cuda())
    torch.cuda.synchronize()
    x, y, ret, st = x.cpu().numpy(), y.cpu().numpy(), ret.cpu().numpy(), stats.cpu().numpy()
    assert (st[:, 15] >= 0).all(), ("the cooperative kernel did not run", st[:, 15].tolist())
    for b, name in enumerate(names):
        r, xo, yo, so = jv.seeded_raw(Cs[b], us[b], vs[b])
        outside = int(st[b, 26])  # kCsOutsidePaths: paths a bail handed to jv_instance_kernel (phase 3)
        print(f"{label} {name}: ret={r} paths={so['paths']} finds={so['finds']} scan_steps={so['scan_steps']} "
              f"handed to phase 3={outside}")
        assert r == int(ret[b]) == 0, (name, r, int(ret[b]), int(st[b, 12]))
        assert np.array_equal(xo, x[b]) and np.array_equal(yo, y[b]), name
        for q, k in ((4, "paths"), (5, "finds"), (6, "scan_steps"), (7, "scan_elems"), (8, "init_elems")):
            assert st[b, q] == so[k], (name, k, int(st[b, q]), so[k])
        if name.startswith("tie"):  # what the instance is there for: at least one hand-over and back
            assert outside >= 1, (name, outside)
    print(f"single-case {label} ok")


if __name__ == "__main__":
    for p in (str(ROOT), str(PKG), str(ROOT / "tests")):
        sys.path.insert(0, p)
    from lap import _hip
    lib = _hip.load()
    print(json.dumps([[lib.lapwarm_coop_members(int(a)), plan_fields(lib, int(a))] for a in sys.argv[1:]]))
