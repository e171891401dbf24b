"""The OneGNN training loss on the MI355X above n = 1024, where the kernels of csrc/train_loss.hip change shape:
the greedy workgroup is capped at 1024 threads (several rows per thread, several trips of every strided loop and
of each bitonic pass), its dynamic LDS passes 64 KiB from n = 4097, the hinge pass gives a wave two rows from
n * B > 8192 (the last one clipped at n_b, whole slots beyond n_b), the 16-byte column pass gets a second column
tile, and a cost matrix that is not 16-byte aligned takes the scalar loads although n % 4 == 0.

The inputs are regenerated from the seeds of train_loss_common.LARGE_SPECS; the expected values are
train_loss_common.restate() at test time, which test_train_loss_fixtures.py pins to the reference at n = 1028.
What is asserted is what test_gpu_train_loss.py asserts at small n, with the same bound: dual_lower, feas, u_reg
and grad_u within 1 float32 ulp of the float64 values (fp64 accumulation, one rounding: the bound does not depend
on n), everything else exact.  Every call here runs with sentinels behind its outputs and in a workspace filled
with 0xA5."""
import numpy as np
import pytest

import train_loss_common as tl
from test_gpu_train_loss import run_abi

pytestmark = pytest.mark.gpu

GOLDEN = tl.TrainLossCases()
GOLDEN_LABELS = GOLDEN.labels()
LARGE = ["uniform-n1025-B8", "uniform-n1028-mixed", "uniform-n4097-B1", "uniform-n4100-mixed", "integer-n1025-B2",
         "inf-n1028-B2"]
TILED = "uniform-n65-mixed-x32"
OUTPUTS = ("v", "arow", "assign", "terms", "grad", "ret")


def golden_case(label):
    m = GOLDEN.case(GOLDEN_LABELS.index(label))
    return dict(cost=m["cost"], u_pred=m["u_pred"], u_target=m["u_target"], sizes=m["sizes"])


def tiled_case(copies=32):
    m = golden_case("uniform-n65-mixed")
    return {k: np.ascontiguousarray(np.concatenate([x] * copies, axis=0)) for k, x in m.items()}


def filled_workspace(B, n):
    """A workspace full of leftovers: a word that is read without being written inside the call shows."""
    import torch

    from lap import _hip
    nbytes = int(_hip.require_device().lapwarm_train_loss_workspace_bytes(B, n))
    assert nbytes > 0
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")


def run(m, **kw):
    return run_abi(m, ws=filled_workspace(*m["u_pred"].shape), tail=True, **kw)


def where_differs(got, want):
    """The first few indices at which two arrays differ in their bits, with both values."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    bad = np.argwhere(np.atleast_1d(got.view(np.int32) != want.astype(got.dtype).view(np.int32)))
    return "; ".join(f"{tuple(int(x) for x in ix)}: got {np.atleast_1d(got)[tuple(ix)]!r} want "
                     f"{np.atleast_1d(want.astype(got.dtype))[tuple(ix)]!r}" for ix in bad[:6]) + f" ({len(bad)} differ)"


def assert_bits(name, got, want):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want, dtype=got.dtype)
    assert got.dtype.itemsize == 4
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), \
        f"{name}: {where_differs(got, want)}"


def assert_one_ulp(name, got, want64):
    """Prints the largest error in float32 ulp, then asserts tl.within_one_ulp."""
    got = np.asarray(got)
    want64 = np.asarray(want64, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - want64) / tl.ulp32(want64)
    print(f"{name}: largest error {err[want64 != 0].max(initial=0.0):.3f} ulp")
    ok = tl.within_one_ulp(got, want64)
    bad = np.argwhere(np.atleast_1d(~ok))
    assert ok.all(), f"{name}: " + "; ".join(
        f"{tuple(int(x) for x in ix)}: got {np.atleast_1d(got)[tuple(ix)]!r} want {np.atleast_1d(want64)[tuple(ix)]!r}"
        for ix in bad[:6]) + f" ({len(bad)} beyond 1 ulp)"


def assert_same_call(got, want, rows=None, keys=OUTPUTS):
    for key in keys:
        a, b = got[key], want[key]
        if rows is not None:
            a, b = a[rows], b[rows]
        assert_bits(key, a, b)


def check_against_restatement(m, r, d):
    sizes = m["sizes"]
    assert (d["ret"] == 0).all(), d["ret"]
    assert_bits("v", d["v"], r["v"])
    assert_bits("arow", d["arow"], r["a"])
    assert_bits("assign", d["assign"], r["assign"])
    assert_bits("primal_upper", d["terms"][:, 3], r["primal_upper"])
    for b, nb in enumerate(sizes):
        assert np.array_equal(np.sort(d["assign"][b, :nb]), np.arange(nb)), (b, "assign is no permutation")
        assert (d["assign"][b, nb:] == -1).all() and (d["arow"][b, nb:] == -1).all(), b
        assert (d["v"][b, nb:] == 0).all() and (d["grad"][b, nb:] == 0).all(), b
    for col, (name, key) in enumerate((("dual_lower", "dual64"), ("feas", "feas64"), ("u_reg", "ureg64"))):
        assert_one_ulp(name, d["terms"][:, col], r[key])
    assert_one_ulp("grad_u", d["grad"], r["g64"])


class Results:
    """Inputs, restatement and device results of each case, made once on first use and never modified."""

    def __init__(self):
        self.made = {}

    def get(self, label):
        if label not in self.made:
            if label == TILED:
                m = tiled_case()
            elif label in tl.LARGE_SPECS:
                m = tl.large_case(label)
            else:
                m = golden_case(label)
            r = tl.restate(m["cost"], m["u_pred"], m["u_target"], m["sizes"])
            self.made[label] = (m, r, run(m))
        return self.made[label]


@pytest.fixture(scope="module")
def results():
    return Results()


@pytest.mark.parametrize("label", LARGE + [TILED])
def test_against_the_restatement(label, results):
    m, r, d = results.get(label)
    check_against_restatement(m, r, d)


def test_cases_are_what_they_are_there_for(results):
    """Properties of the inputs that the cases were chosen for; nothing of the device."""
    m, r, _ = results.get("integer-n1025-B2")
    for b, nb in enumerate(m["sizes"]):
        cm = m["cost"][b, :nb, :nb] - m["u_pred"][b, :nb, None]
        assert ((cm == cm.min(axis=0)).sum(axis=0) > 1).any()
    m, r, _ = results.get("inf-n1028-B2")
    assert np.isinf(m["cost"][0, :1028, :1028]).any() and np.isfinite(r["v"]).all()
    assert np.isfinite(r["g64"]).all() and np.isfinite(r["feas64"]).all()


def test_tiled_copies_have_the_bits_of_the_small_batch(results):
    """128 instances of n = 65: a wave of the hinge pass owns two rows, with n_b = 1 and 33 among the sizes and
    batch indices up to 127.  Every copy gives what the B = 4 call gives; grad_u carries another 1 / B."""
    m, r, d = results.get(TILED)
    _, _, small = results.get("uniform-n65-mixed")
    for c in range(32):
        rows = slice(4 * c, 4 * c + 4)
        for key in ("v", "arow", "assign", "terms"):
            assert_bits(f"copy {c} {key}", d[key][rows], small[key])
    assert_one_ulp("grad_u", d["grad"], r["g64"])


@pytest.mark.parametrize("label", ["uniform-n64-B3", "uniform-n1028-mixed"])
def test_cost_that_is_not_16_byte_aligned(label, results):
    """n % 4 == 0 with C 4 bytes into its allocation: the scalar loads, and the bits of the aligned call."""
    m, _, d = results.get(label)
    assert m["u_pred"].shape[1] % 4 == 0
    e = run(m, cost_offset=4)
    assert_same_call(e, d)


def test_through_gnn_losses_aligned_and_offset(results):
    """warmstart_loss and greedy_primal_upper_batch on uniform-n1028-mixed: the metrics have the bits of the
    direct call, u.grad those of the backward call with the weights (1, 1, 0.1); the same from a cost that is
    a view 4 bytes into its storage, which cost.contiguous() leaves where it is."""
    import torch

    from gnn.losses import greedy_primal_upper_batch, warmstart_loss
    m, _, d = results.get("uniform-n1028-mixed")
    dev = torch.device("cuda:0")
    B, n = m["u_pred"].shape
    target = torch.from_numpy(m["u_target"]).to(dev)
    mask = torch.arange(n, device=dev)[None, :] < torch.from_numpy(m["sizes"].astype(np.int64)).to(dev)[:, None]
    aligned = torch.from_numpy(m["cost"]).to(dev)
    buf = torch.empty((B * n * n + 1,), dtype=torch.float32, device=dev)
    shifted = buf[1:].view(B, n, n)
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    gap = d["terms"][:, 3] - d["terms"][:, 0]
    for name, cost in (("aligned", aligned), ("offset", shifted)):
        u = torch.from_numpy(m["u_pred"]).to(dev).requires_grad_()
        loss, metrics = warmstart_loss(cost, u, target, mask)
        loss.backward()
        got = {k: x.detach().cpu().numpy() for k, x in metrics.items()}
        assert_bits(f"{name} v_proj", got["v_proj"], d["v"])
        assert_bits(f"{name} argmin_row", got["argmin_row"], d["arow"])
        assert_bits(f"{name} assign", got["assign"], d["assign"])
        assert_bits(f"{name} ret", got["ret"], d["ret"])
        for col, key in enumerate(("dual_lower", "feas", "u_reg", "primal_upper")):
            assert_bits(f"{name} {key}", got[key], d["terms"][:, col])
        assert_bits(f"{name} primal_gap", got["primal_gap"], gap)
        assert_bits(f"{name} u.grad", u.grad.cpu().numpy(), d["grad"])
        pu, assign = greedy_primal_upper_batch(cost, u.detach(), mask)
        assert_bits(f"{name} greedy primal_upper", pu.cpu().numpy(), d["terms"][:, 3])
        assert_bits(f"{name} greedy assign", assign.cpu().numpy(), d["assign"])


def test_bad_size_beside_large_neighbours(results):
    m, _, d = results.get("uniform-n1028-mixed")
    B, n = m["u_pred"].shape
    keep = [b for b in range(B) if b != 3]
    for bad in (0, n + 1):
        sizes = m["sizes"].copy()
        sizes[3] = bad
        e = run(m, sizes=sizes)
        assert e["ret"].tolist() == [0, 0, 0, 2, 0, 0, 0, 0]
        assert np.isnan(e["terms"][3]).all()
        assert (e["assign"][3] == -1).all() and (e["grad"][3] == 0).all()
        assert_same_call(e, d, rows=keep)


def test_other_stream_reusing_the_workspace_at_n4097(results):
    """The same bits from a second call on another stream in the workspace the first call left behind."""
    import torch
    m, _, d = results.get("uniform-n4097-B1")
    e = run_abi(m, stream=torch.cuda.Stream(torch.device("cuda:0")), ws=d["ws"], tail=True)
    assert_same_call(e, d)
