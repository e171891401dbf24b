"""GPU tests (-m gpu): every instantiation of the cooperative shortest-path kernel (coop_ssp_kernel<CH, NL>,
csrc/coop_ssp.hip) and every switch that changes its code paths or the helper workgroups', against the CPU
oracle.  The configurations are the rows of tests/coop_configs_common.py (test_host_logic.py checks on the CPU
that the planner plans them).  A row runs the native driver's whole sweep at its one size -- ten cost
families x the seed kinds the driver pairs with them + nine cold solves, the tie-heavy families that make
the kernel bail and hand a path to jv_instance_kernel (phase 3) included -- in a child process, because the
switches are read once per process.  Every child runs under its own time limit and is never retried: the
kernel polls mailboxes, so a wrong instantiation is more likely to spin than to answer wrongly."""
import os
import subprocess
import sys

import pytest

import coop_configs_common as cc

pytestmark = pytest.mark.gpu

SWEEPS = [c for c in cc.CONFIGS if c.runs == "sweep"]


@pytest.mark.parametrize("cfg", SWEEPS, ids=[c.label for c in SWEEPS])
def test_cooperative_instantiation_native_sweep(cfg):
    """One (CH, NL) at one size, mostly with a last member that holds one position: bit-exact on all 58
    cases, and the progress line says the cooperative kernel was planned with the row's member count (a
    forced geometry without an instantiation falls back to the one-workgroup path silently)."""
    seen, _ = cc.run_sweep(cfg.env, (cfg.n,), cfg.timeout)
    assert seen == {cfg.n: cfg.members}, seen


@pytest.mark.parametrize("sweep", cc.SWITCH_SWEEPS, ids=[s.label for s in cc.SWITCH_SWEEPS])
def test_switch_native_sweep(sweep):
    """LAPWARM_COOP_XCD_STORES=0 (agent-scope mailbox stores), LAPWARM_COOP_RELAUNCHES=0 / 1 (phase 2 finishes
    every path left after the first bail / after one hand-over and back; the tie families bail early, so it
    starts with many free rows) and LAPWARM_HELPERS_PER_INSTANCE=4 / 2 (the driver solves one instance per
    call, so the helpers are launched): the whole sweep at a few sizes, bit-exact."""
    seen, _ = cc.run_sweep(sweep.env, sweep.sizes, sweep.timeout)
    assert seen == dict(zip(sweep.sizes, sweep.members)), seen


_SINGLE_CASE = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import coop_configs_common as cc
cc.run_single_case(sys.argv[1])
"""


def test_ch16_two_load_poll_single_case():
    """c16_11: n = 10241 with LAPWARM_COOP_CH=16 -- 11 members of 1024 positions, the only class that reaches
    coop_ssp_kernel<16, 2>, last member one position.  One uniform instance with float32-rounded row-min seeds
    (the driver's `rowmin32` recipe): x, y, ret bit-equal and the counters equal to the oracle's.  Measured: all
    2261 paths of that instance end inside the cooperative kernel -- its ties are of the kinds the kernel
    handles itself -- so a tie-family instance with row-min seeds runs beside it: 96 paths handed to phase 3
    and back, the rest finished by phase 2 (asserted: at least one hand-over).  About a minute, most of it the
    tie instance (oracle 23 s).  A child process: the switch has to be set before the library loads."""
    cfg = {c.label: c for c in cc.CONFIGS}["c16_11"]
    script = _SINGLE_CASE % (str(cc.ROOT), str(cc.PKG), str(cc.ROOT / "tests"))
    proc = subprocess.run([sys.executable, "-c", script, cfg.label], capture_output=True, text=True,
                          timeout=cfg.timeout, env=dict(os.environ, **cfg.env), cwd=str(cc.ROOT))
    print(proc.stdout[-1500:])
    assert proc.returncode == 0 and "single-case c16_11 ok" in proc.stdout, (proc.returncode, proc.stdout[-2000:],
                                                                           proc.stderr[-3000:])


def test_ch4_three_load_poll_single_cases():
    """c4_27: n = 6657 in the default environment -- 27 members of 256 positions, the first three-load poll
    (coop_ssp_kernel<4, 3>), an odd n (no 16-byte row prefetch), last member one position.  A uniform instance
    with float32-rounded seeds and a sparse one with row-min seeds (measured: neither hands a path to phase 3)
    beside a tie-family one that does (asserted: at least once): bit-equal, and the path / collection /
    relax-step / element counters of the kernels that took part add up to the oracle's."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    cc.run_single_case("c4_27")
