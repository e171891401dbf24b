"""The training-loss fixtures (tests/golden/train_loss_cases.npz, written from the reference by
tests/golden/make_train_loss.py) against the NumPy restatement of train_loss_common.py, the C header and the
argument checks of gnn.losses; and the restatement at n = 1028, on inputs regenerated from their seeds, against the
reference's recorded results in tests/golden/train_loss_large_ref.npz.  No GPU."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

import train_loss_common as tl

ROOT = Path(__file__).resolve().parents[1]
CASES = tl.TrainLossCases()
ALL = list(range(len(CASES)))
LABELS = CASES.labels()
GRADIENT = [k for k in ALL if CASES.meta[k]["kind"] == "uniform"]


def test_cases_cover_the_shapes():
    shapes = {(m["n"], m["B"]) for m in CASES.meta if m["kind"] == "uniform"}
    assert {(n, B) for n in (1, 2, 7, 63, 64, 65, 257) for B in (1, 3)} <= shapes
    mixed = [k for k in ALL if LABELS[k].endswith("mixed")]
    assert len(mixed) == 2
    for k in mixed:
        assert CASES.case(k)["sizes"].tolist() == [65, 64, 1, 33]
    assert any(m["kind"] == "integer" for m in CASES.meta)


@pytest.mark.parametrize("k", ALL, ids=LABELS)
def test_restatement_reproduces_the_stored_fields(k):
    m, r = CASES.case(k), CASES.restated(k)
    assert tl.bits_equal32(r["v"], m["ref_v"])
    assert np.array_equal(r["assign"], m["assign"])
    assert tl.bits_equal32(r["primal_upper"], m["primal_stable"])
    # The float64 fields were stored from this same restatement: comparing them only guards against drift of
    # train_loss_common.py after the file was written.  The independent check of the restatement is
    # test_reference_sums_and_gradient_within_the_summation_bound, against the reference's own numbers.
    for key in ("dual64", "feas64", "ureg64", "g64"):
        assert np.array_equal(r[key], m[key]), key
    if m["primal_equal"]:
        assert tl.bits_equal32(r["primal_upper"], m["ref_primal"])
    # every row has a column, every column of the instance is used once
    for b, nb in enumerate(m["sizes"]):
        assert sorted(r["assign"][b, :nb].tolist()) == list(range(nb))
        assert (r["assign"][b, nb:] == -1).all()


@pytest.mark.parametrize("k", GRADIENT, ids=[LABELS[k] for k in GRADIENT])
def test_reference_sums_and_gradient_within_the_summation_bound(k):
    m, r = CASES.case(k), CASES.restated(k)
    bound = tl.reference_bounds(r, m["sizes"])
    assert (np.abs(m["ref_dual"] - r["dual64"]) <= bound["dual"]).all()
    assert (np.abs(m["ref_feas"] - r["feas64"]) <= bound["feas"]).all()
    assert (np.abs(m["ref_ureg"] - r["ureg64"]) <= bound["ureg"]).all()
    assert (np.abs(m["ref_grad"] - r["g64"]) <= bound["grad"]).all()
    # the reference's gradient is 0 on padded rows, and so is the closed form
    for b, nb in enumerate(m["sizes"]):
        assert (m["ref_grad"][b, nb:] == 0).all() and (r["g64"][b, nb:] == 0).all()


def test_large_specs_reach_the_paths_they_are_there_for():
    """The shapes of the cases above n = 1024, restated from csrc/train_loss.hip's launch arithmetic."""
    def plan(B, n):
        rows = max(1, -(-n * B // 8192))
        p2 = 1 << (n - 1).bit_length()
        return dict(rows_per_wave=rows, hparts=-(-n // (rows * 4)) * 4, p2=p2, lds=8 * p2 + 4 * -(-n // 32))
    spec = tl.LARGE_SPECS
    assert plan(8, 1025)["rows_per_wave"] == 2 and plan(8, 1028)["rows_per_wave"] == 2
    assert plan(3, 4100)["rows_per_wave"] == 2 and plan(128, 65)["rows_per_wave"] == 2
    one = plan(1, 4097)
    assert one == dict(rows_per_wave=1, hparts=4100, p2=8192, lds=66052)
    assert spec["uniform-n4097-B1"][2:4] == (1, 4097) and spec["uniform-n4100-mixed"][2:4] == (3, 4100)
    assert spec["uniform-n1028-mixed"][4] == [1028, 1025, 1, 513, 1024, 64, 1027, 1000]
    assert spec["uniform-n4100-mixed"][4] == [4100, 4097, 2049]
    assert len({s[1] for s in spec.values()}) == len(spec)  # a seed of its own each
    for label in tl.LARGE_REF_LABELS:
        assert spec[label][2:] == (2, 1028, [1028, 1025])


@pytest.mark.parametrize("label", tl.LARGE_REF_LABELS)
def test_restatement_against_the_reference_at_n1028(label):
    """restate() is the expected value of every test of test_gpu_train_loss_large.py: here it meets what the
    reference computed at n = 1028, uniform and with isolated +inf entries."""
    z = np.load(tl.LARGE_REF, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    k = [m["label"] for m in meta].index(label)
    m = tl.large_case(label)
    assert meta[k]["seed"] == m["seed"] and (meta[k]["B"], meta[k]["n"]) == m["u_pred"].shape
    assert tl.input_crc(m) == meta[k]["crc"], (
        "the regenerated inputs differ from the ones the fixture was recorded on: this NumPy's random stream "
        f"(numpy {np.__version__}) differs, not the kernel or the restatement")
    if m["kind"] == "inf":
        frac = np.mean([np.isinf(m["cost"][b, :nb, :nb]).mean() for b, nb in enumerate(m["sizes"])])
        assert 0.09 < frac < 0.11
    r = tl.restate(m["cost"], m["u_pred"], m["u_target"], m["sizes"])
    assert tl.bits_equal32(r["v"], z[f"c{k}_ref_v"])
    bound = tl.reference_bounds(r, m["sizes"])
    assert (np.abs(z[f"c{k}_ref_dual"] - r["dual64"]) <= bound["dual"]).all()
    assert (np.abs(z[f"c{k}_ref_feas"] - r["feas64"]) <= bound["feas"]).all()
    assert (np.abs(z[f"c{k}_ref_ureg"] - r["ureg64"]) <= bound["ureg"]).all()
    assert (np.abs(z[f"c{k}_ref_grad"] - r["g64"]) <= bound["grad"]).all()
    assert np.isfinite(r["v"]).all() and np.isfinite(r["g64"]).all() and (r["feas64"] > 0).all()
    for b, nb in enumerate(m["sizes"]):
        assert (z[f"c{k}_ref_grad"][b, nb:] == 0).all() and (r["g64"][b, nb:] == 0).all()
        assert sorted(r["assign"][b, :nb].tolist()) == list(range(nb))


def test_integer_cases_are_tied():
    """The integer cases exist for their ties: in each, some column minimum is attained by two rows."""
    for k in ALL:
        m = CASES.case(k)
        if m["kind"] != "integer" or m["n"] < 7:  # two rows of n = 2 need not tie
            continue
        tied = False
        for b, nb in enumerate(m["sizes"]):
            cm = m["cost"][b, :nb, :nb] - m["u_pred"][b, :nb, None]
            tied |= bool(((cm == cm.min(axis=0)).sum(axis=0) > 1).any())
        assert tied, LABELS[k]


def test_ulp_helper():
    one = np.float64(1.0)
    assert tl.ulp32(one) == 2.0 ** -23 and tl.ulp32(0.75) == 2.0 ** -24
    assert tl.within_one_ulp(np.float32(1.0) + np.float32(2.0 ** -23), one)
    assert not tl.within_one_ulp(np.float32(1.0) + np.float32(2.0 ** -22), one)
    assert tl.within_one_ulp(np.float32(0.0), 0.0) and not tl.within_one_ulp(np.float32(1e-45), 0.0)


def test_header_declares_the_symbols():
    header = (ROOT / "include" / "lapwarm_hip.h").read_text()
    from lap import _hip
    for name in ("lapwarm_train_loss_workspace_bytes", "lapwarm_train_loss_forward", "lapwarm_train_loss_backward"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _hip.SIGNATURES
    assert "train_one_gnn.py:180-226" in header and ":137-177" in header


def test_losses_rejects_bad_arguments_before_the_device(monkeypatch):
    import torch

    import gnn
    from gnn import losses
    from lap import _hip

    assert "losses" not in gnn.__all__ and callable(losses.warmstart_loss)
    assert losses.__all__ == ["warmstart_loss", "greedy_primal_upper_batch"]

    def no_device():
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_hip, "require_device", no_device)
    monkeypatch.setattr(_hip, "load", no_device)
    B, n = 2, 5
    cost = torch.zeros(B, n, n)
    u = torch.zeros(B, n)
    mask = torch.ones(B, n, dtype=torch.bool)
    with pytest.raises(TypeError, match="cost must be torch.float32"):
        losses.warmstart_loss(cost.double(), u, u, mask)
    with pytest.raises(TypeError, match="mask must be torch.bool"):
        losses.warmstart_loss(cost, u, u, mask.float())
    with pytest.raises(TypeError, match="u_target must be torch.float32"):
        losses.warmstart_loss(cost, u, u.double(), mask)
    with pytest.raises(TypeError, match="torch.Tensor"):
        losses.warmstart_loss(cost.numpy(), u, u, mask)
    with pytest.raises(ValueError, match=r"cost must be \(B, n, n\)"):
        losses.warmstart_loss(torch.zeros(B, n, n + 1), u, u, mask)
    with pytest.raises(ValueError, match=r"u_pred must be \(2, 5\)"):
        losses.warmstart_loss(cost, torch.zeros(B, n + 1), u, mask)
    with pytest.raises(ValueError, match=r"mask must be \(2, 5\)"):
        losses.warmstart_loss(cost, u, u, mask[:1])
    with pytest.raises(ValueError, match="16384"):
        losses.greedy_primal_upper_batch(torch.zeros(1, 1, 1).expand(1, 16385, 16385), torch.zeros(1, 16385))
    with pytest.raises(ValueError, match="must be on the GPU"):
        losses.warmstart_loss(cost, u, u, mask)
    with pytest.raises(ValueError, match="must be on the GPU"):
        losses.greedy_primal_upper_batch(cost, u)
    with pytest.raises(ValueError, match="weights"):
        losses.warmstart_loss(cost, u, u, mask, weights=(1.0, 1.0))
