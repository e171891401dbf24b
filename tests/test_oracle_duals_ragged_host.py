"""The ragged oracle duals without a GPU: the ABI surface of lapwarm_oracle_duals_ragged, its argument errors and
workspace query, and a NumPy model of its driver -- a chunk schedule shared by the batch, a sweep budget and a
`last` check per instance -- which must leave every instance exactly where the uniform driver leaves it alone."""
import ctypes as ct

import numpy as np
import pytest

from host_common import lib  # noqa: F401
from oracle_duals_common import jacobi, make_C, oracle_from_v
from oracle_duals_ragged_common import chain_instance, hungarian, model_alone, model_ragged, run_driver, Instance

SIZES = (2, 5, 7, 13, 37, 64)


def test_workspace_query(lib):
    q, uniform = lib.lapwarm_oracle_duals_ragged_workspace_bytes, lib.lapwarm_oracle_duals_workspace_bytes
    assert q(1, 0) == 0 and q(0, 64) == 0 and q(-1, 64) == 0 and q(4, -1) == 0
    assert q(1, 16385) == 0 and q(65536, 8) == 0
    for B, N in ((1, 1), (3, 37), (32, 640), (4, 2049), (1, 16384)):
        assert q(B, N) == uniform(B, N) > 0  # one layout function: the uniform slots with the padded stride


def test_argument_errors_return_before_any_device_work(lib):
    call = lib.lapwarm_oracle_duals_ragged
    dev = 1 << 20  # never dereferenced
    ws_bytes = lib.lapwarm_oracle_duals_ragged_workspace_bytes(3, 300)
    good = dict(C=dev, offsets=dev, sizes=dev, host_sizes=(ct.c_int * 3)(5, 64, 300), ld=0, batch=3, N=300,
                rows=dev, cols=dev, u=dev, v=dev, ret=dev, sweeps=None, ws=dev, ws_bytes=ws_bytes, stream=None)

    def rc(**change):
        a = dict(good, **change)
        return call(a["C"], a["offsets"], a["sizes"], a["host_sizes"], a["ld"], a["batch"], a["N"], a["rows"],
                    a["cols"], a["u"], a["v"], a["ret"], a["sweeps"], a["ws"], a["ws_bytes"], a["stream"])

    assert rc(batch=0) == -2 and rc(batch=-1) == -2 and rc(batch=65536) == -2
    assert rc(N=0) == -2 and rc(N=-5) == -2 and rc(ld=-1) == -2
    assert rc(N=16385) == -5
    for name in ("C", "offsets", "sizes", "host_sizes", "rows", "cols", "u", "v", "ret", "ws"):
        assert rc(**{name: None}) == -2, name
    assert rc(ws_bytes=ws_bytes - 1) == -1


# ---- the model of the driver ----

def uniform_pair(n, seed=3):
    C = make_C(("uniform", n, seed))
    return C, hungarian(C)


def chain_pair(n):
    return chain_instance(n), np.arange(n)


def test_hungarian_is_optimal_on_small_instances():
    from itertools import permutations
    for n in (1, 2, 5, 7):
        C = make_C(("uniform", n, 11))
        best = min(permutations(range(n)), key=lambda p: C[np.arange(n), list(p)].sum())
        assert list(hungarian(C)) == list(best)


@pytest.mark.parametrize("n", (7, 13, 37))
def test_chain_instance_outlasts_its_budget_and_is_feasible(n):
    C, x = chain_pair(n)
    v, sweeps = jacobi(C, x, x)
    assert sweeps == n  # n - 1 updating sweeps: not settled within the n - 1 of the budget
    u, v = oracle_from_v(C, x, x, v)
    red = (C - u[:, None]) - v[None, :]
    assert red.min() == 0.0 and np.all(red[x, x] == 0.0)
    v_model, made, replay = model_alone(C, x)
    assert made == n - 1 and replay  # handed to the replay through `last`


def test_uniform_instances_settle_in_the_model_as_jacobi_does():
    for n in SIZES:
        C, x = uniform_pair(n)
        vj, sj = jacobi(C, np.arange(n), x)
        v, made, replay = model_alone(C, x)
        if sj <= n - 1:
            assert not replay and made == sj and np.array_equal(v, vj), n
        else:
            assert replay and made == n - 1, n


BATCHES = {
    "uniform": [uniform_pair(n) for n in SIZES],
    "chains": [chain_pair(n) for n in SIZES],
    "mixed_chains_first": [chain_pair(7), chain_pair(13), chain_pair(37), uniform_pair(2), uniform_pair(5),
                           uniform_pair(64)],
    "mixed_alternating": [uniform_pair(64), chain_pair(7), uniform_pair(13), chain_pair(37), uniform_pair(2),
                          chain_pair(13), uniform_pair(7), chain_pair(5), uniform_pair(37), chain_pair(2)],
    "non_optimal": [uniform_pair(64), (uniform_pair(37)[0], np.roll(uniform_pair(37)[1], 1)), chain_pair(7),
                    (uniform_pair(13)[0], np.roll(uniform_pair(13)[1], 1))],
}


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_every_instance_of_a_ragged_batch_ends_where_it_ends_alone(name):
    pairs = BATCHES[name]
    got = model_ragged(pairs)
    for (C, x), (v, made, replay) in zip(pairs, got):
        va, made_a, replay_a = model_alone(C, x)
        assert np.array_equal(v.view(np.int64), va.view(np.int64)), (name, C.shape[0])
        assert (made, replay) == (made_a, replay_a), (name, C.shape[0])


def test_budgets_that_end_inside_a_shared_chunk():
    """The shared checks come after sweeps 4, 12, 28, 60: n = 7 (budget 6) and n = 37 (budget 36) end inside a
    chunk and n = 13 (budget 12) at the end of one; beside n = 64 each is frozen at its budget and handed on at
    the next shared check."""
    pairs = [chain_pair(7), chain_pair(13), chain_pair(37), chain_pair(64)]
    ts = [Instance(C, x) for C, x in pairs]
    checks = run_driver(ts, ragged=True)
    assert [t.sweeps for t in ts] == [6, 12, 36, 63]
    assert all(t.result()[2] for t in ts)
    alone = [Instance(*pairs[-1])]
    assert checks == run_driver(alone, ragged=False)  # as many synchronisations as the largest instance alone


def test_a_host_budget_below_the_instance_budget_still_ends_the_instance():
    """The schedule runs to the host's budget.  An instance whose own budget lies beyond it (a device size above
    every host size) and that has not settled is handed on by the host's `last`: it does not stay running."""
    ts = [Instance(*chain_pair(37)), Instance(*uniform_pair(13))]
    run_driver(ts, ragged=True, max_s=19)
    v, made, replay = ts[0].result()
    assert made == 19 and replay
    assert ts[1].result()[2] == model_alone(*uniform_pair(13))[2]
