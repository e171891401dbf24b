"""Oracle duals on the MI355X against the reference's outcomes (tests/golden/oracle_duals_cases.npz):
the drop-in, compute_oracle_duals / make_feasible_duals, check_dual_and_match and the batched
device API."""
import contextlib
import ctypes as ct
import io
import time

import numpy as np
import pytest

from host_common import bits_equal, small_model_pipe as pipe  # noqa: F401
from oracle_duals_common import OracleCases, jacobi, oracle_from_v, sha

pytestmark = pytest.mark.gpu

CASES = OracleCases()
DIFF = CASES.indices("diff")
ORACLE = CASES.indices("oracle")
FEASIBLE = CASES.indices("feasible")


@pytest.mark.parametrize("k", DIFF, ids=[CASES.meta[k]["label"] for k in DIFF])
def test_drop_in_matches_reference(k):
    from solvers import dual_from_matching_diff_constraints
    m = CASES.case(k)
    if m["outcome"] == "ok":
        u, v, red = dual_from_matching_diff_constraints(m["C"], m["rows"], m["cols"])
        assert bits_equal(u, m["u"]) and bits_equal(v, m["v"])
        assert sha(red) == m["sha_red"]
    else:
        exc = RuntimeError if m["outcome"] == "RuntimeError" else AssertionError
        with pytest.raises(exc) as ei:
            dual_from_matching_diff_constraints(m["C"], m["rows"], m["cols"])
        assert type(ei.value) is exc and str(ei.value) == m["message"]


@pytest.mark.parametrize("k", ORACLE, ids=[CASES.meta[k]["label"] for k in ORACLE])
def test_compute_oracle_duals_matches_reference(k):
    import lap
    from solvers import compute_oracle_duals
    m = CASES.case(k)
    _, x, _ = lap.lapjv(m["C"])
    assert np.array_equal(x, m["cols"])
    np.random.seed(123)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        u, v = compute_oracle_duals(m["C"], noise_level=m["noise"])
    assert ("Warning: Difference constraints failed" in buf.getvalue()) == m["fallback"]
    assert buf.getvalue() == m["printed"]
    assert bits_equal(u, m["u"]) and bits_equal(v, m["v"])
    # the global RNG is left as the reference leaves it
    got = np.random.get_state()
    np.random.seed(123)
    if m["noise"] > 0:
        np.random.seed(42)
        np.random.normal(0, m["noise"], m["n"])
        np.random.normal(0, m["noise"], m["n"])
    want = np.random.get_state()
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:] == want[2:]


@pytest.mark.parametrize("k", FEASIBLE, ids=[CASES.meta[k]["label"] for k in FEASIBLE])
def test_make_feasible_duals_matches_reference(k):
    import lap
    from solvers import make_feasible_duals
    m = CASES.case(k)
    _, x, _ = lap.lapjv(m["C"])
    assert np.array_equal(x, m["cols"])
    u, v = make_feasible_duals(m["C"], noise_std=m["noise_std"])
    assert bits_equal(u, m["u"]) and bits_equal(v, m["v"])


@pytest.mark.parametrize("n", [64, 256])
def test_ties_give_valid_duals(n):
    import lap
    from solvers import check_dual_and_match, compute_oracle_duals, make_feasible_duals
    C = np.random.RandomState(n).randint(1, 101, size=(n, n)).astype(np.float64)
    _, x, _ = lap.lapjv(C)
    u, v = compute_oracle_duals(C)
    assert check_dual_and_match(C, u, v, np.arange(n), x)
    u2, v2 = make_feasible_duals(C)
    red = C - u2[:, None] - v2[None, :]
    assert red.min() >= -1e-8


def test_check_dual_and_match_pass_and_fail():
    import lap
    from solvers import check_dual_and_match, compute_oracle_duals
    from solvers.generators import generate_family
    C = generate_family("uniform", 128, 5)
    _, x, _ = lap.lapjv(C)
    rows = np.arange(128)
    u, v = compute_oracle_duals(C)
    assert check_dual_and_match(C, u, v, rows, x) is True
    with pytest.raises(AssertionError, match="^Dual infeasible: some reduced costs < 0$"):
        check_dual_and_match(C, u + 1e-3, v, rows, x)
    with pytest.raises(AssertionError, match="^Complementary slackness violated on matched edges$"):
        check_dual_and_match(C, u - 1e-3, v, rows, x)


def test_verify_solver_correctness():
    from solvers import compute_oracle_duals, verify_solver_correctness
    from solvers.generators import generate_family
    C = generate_family("uniform", 96, 2)
    u, v = compute_oracle_duals(C)
    assert verify_solver_correctness(C, u, v) is True


def test_batched_matches_drop_in_and_restatement(pipe):
    import torch

    from solvers import dual_from_matching_diff_constraints
    from solvers.generators import mixed_batch
    fams = ("uniform", "sparse", "tie", "noisy_linear", "metric", "low_rank", "clustered", "block")
    C_host, labels = mixed_batch(32, 2048, families=fams, seed=17)
    C = torch.from_numpy(C_host).to("cuda:0")
    x, u, v, ret, sweeps = pipe.oracle_duals_batch(C)
    torch.cuda.synchronize()
    x, u, v = x.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy()
    ret, sweeps = ret.cpu().numpy(), sweeps.cpu().numpy()
    assert (ret == 0).all(), (ret, labels)
    rows = np.arange(2048)
    for b in range(32):
        ub, vb, _ = dual_from_matching_diff_constraints(C_host[b], rows, x[b])
        assert bits_equal(u[b], ub) and bits_equal(v[b], vb), labels[b]
    for b in (labels.index("uniform"), labels.index("sparse")):
        vj, sj = jacobi(C_host[b], rows, x[b])
        uj, vj = oracle_from_v(C_host[b], rows, x[b], vj)
        assert bits_equal(u[b], uj) and bits_equal(v[b], vj), labels[b]
        assert sweeps[b, 0] == sj and sweeps[b, 1] == sj - 1 and sweeps[b, 3] == 0, (labels[b], sweeps[b], sj)
    # a seeded solve from the oracle duals finds the cold lapjv assignment, or an equally cheap one
    # where the optimum is not unique (exact zeros of the clamped families, near-ties of `tie`)
    xs, _, rs, _ = pipe.seeded_batch(C, torch.from_numpy(u).to("cuda:0"), torch.from_numpy(v).to("cuda:0"))
    torch.cuda.synchronize()
    assert (rs.cpu().numpy() == 0).all()
    xs = xs.cpu().numpy()
    for b in range(32):
        if labels[b] in ("uniform", "sparse", "noisy_linear"):
            assert np.array_equal(xs[b], x[b].astype(np.int64)), labels[b]
        else:
            c_seeded = C_host[b][rows, xs[b]].sum()
            c_cold = C_host[b][rows, x[b]].sum()
            assert abs(c_seeded - c_cold) <= 1e-9 * max(1.0, abs(c_cold)), labels[b]


def test_n16384_uniform_finishes_feasible(pipe):
    import torch

    n = 16384
    g = torch.Generator(device="cuda:0").manual_seed(3)
    C = torch.rand((1, n, n), dtype=torch.float64, device="cuda:0", generator=g)
    t0 = time.time()
    x, u, v, ret, sweeps = pipe.oracle_duals_batch(C)
    torch.cuda.synchronize()
    assert int(ret[0]) == 0, (int(ret[0]), sweeps.cpu().numpy())
    # device feasibility check: the row minima of C - v, less u
    rmin = torch.empty((1, n), dtype=torch.float64, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rc = pipe.lib.lapwarm_rowmin_batched(C.data_ptr(), 1, n, v.data_ptr(), rmin.data_ptr(), ct.c_void_p(stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert float((rmin - u).min()) >= -1e-8
    print(f"n=16384 uniform: {time.time() - t0:.2f} s, sweeps {sweeps.cpu().numpy().tolist()}")


@pytest.mark.parametrize("n", [512, 8192])
def test_non_optimal_matching_raises_quickly(n):
    import lap
    from solvers import dual_from_matching_diff_constraints
    from solvers.generators import generate_family
    C = generate_family("uniform", n, 21)
    _, x, _ = lap.lapjv(C)
    t0 = time.time()
    with pytest.raises(RuntimeError, match="^Negative cycle while solving difference constraints for v.$"):
        dual_from_matching_diff_constraints(C, np.arange(n), np.roll(x, 1))
    assert time.time() - t0 < 30.0


def test_bad_inputs_raise_value_error():
    from solvers import dual_from_matching_diff_constraints
    C = np.random.default_rng(0).uniform(size=(6, 6))
    r = np.arange(6)
    with pytest.raises(ValueError):
        dual_from_matching_diff_constraints(C[:, :5], r[:5], r[:5])
    with pytest.raises(ValueError):
        dual_from_matching_diff_constraints(C, r[:4], r[:4])
    with pytest.raises(ValueError):
        dual_from_matching_diff_constraints(C, r, np.array([0, 1, 2, 3, 4, 4]))
    with pytest.raises(ValueError):
        dual_from_matching_diff_constraints(C, r, np.array([0, 1, 2, 3, 4, 6]))
    for bad in (np.nan, np.inf):
        Cb = C.copy()
        Cb[2, 3] = bad
        with pytest.raises(ValueError):
            dual_from_matching_diff_constraints(Cb, r, r)
