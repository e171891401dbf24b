"""The DualGNN-loss fixtures (tests/golden/dual_loss_cases.npz, written from the reference by
tests/golden/make_dual_loss.py) against the NumPy restatement of dual_loss_common.py; the three C entries in the
binding, the header and the library, their workspace size and their argument codes (the never-followed pointer of
abi_contract_common.py); and the argument checks of gnn.losses.dual_warmstart_loss.  No GPU."""
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest

import abi_contract_common as acc
import dual_loss_common as dl
import train_loss_common as tl
from host_common import lib  # noqa: F401

ROOT = Path(__file__).resolve().parents[1]
CASES = dl.DualLossCases()
ALL = list(range(len(CASES)))
LABELS = CASES.labels()
GRADIENT = [k for k in ALL if CASES.meta[k]["kind"] == "uniform"]
SYMBOLS = ("lapwarm_dual_loss_workspace_bytes", "lapwarm_dual_loss_forward", "lapwarm_dual_loss_backward")


def test_cases_cover_the_sizes():
    assert {m["n"] for m in CASES.meta if m["kind"] == "uniform"} == {1, 5, 33, 64, 257}
    mixed = {LABELS[k]: CASES.case(k)["sizes"].tolist() for k in ALL if LABELS[k].endswith("mixed")}
    assert mixed["uniform-n64-mixed"] == [64, 33, 1, 5] and mixed["uniform-n257-mixed"] == [257, 130]
    assert any(m["kind"] == "integer" for m in CASES.meta)
    assert dl.GOLDEN.stat().st_size < 1 << 20


@pytest.mark.parametrize("k", ALL, ids=LABELS)
def test_restatement_reproduces_the_exact_fields(k):
    m, r = CASES.case(k), CASES.restated(k)
    assert tl.bits_equal32(r["v"], m["ref_v"])
    one = tl.restate(m["cost"], m["u_pred"], m["v_hint"], m["sizes"])  # the OneGNN restatement of the same inputs
    assert np.array_equal(r["a"], one["a"]) and np.array_equal(r["assign"], one["assign"])
    assert tl.bits_equal32(r["primal_upper"], one["primal_upper"])
    if m["primal_equal"]:
        assert tl.bits_equal32(r["primal_upper"], m["ref_primal"])
    for b, nb in enumerate(m["sizes"]):
        assert sorted(r["assign"][b, :nb].tolist()) == list(range(nb)) and (r["assign"][b, nb:] == -1).all()
        assert (r["a"][b, nb:] == -1).all() and ((r["a"][b, :nb] >= 0) & (r["a"][b, :nb] < nb)).all()
        # S_i is the sum of d over the columns row i owns
        for i in range(nb):
            own = np.flatnonzero(r["a"][b, :nb] == i)
            assert r["cnt"][b, i] == len(own)
            assert r["S"][b, i] == sum((float(r["d"][b, j]) for j in own), 0.0)


@pytest.mark.parametrize("k", GRADIENT, ids=[LABELS[k] for k in GRADIENT])
def test_reference_terms_and_gradients_within_the_summation_bound(k):
    m, r = CASES.case(k), CASES.restated(k)
    assert dl.untied(m["cost"], m["u_pred"], r["v"], m["sizes"]) == m["rows_untied"]
    for b, nb in enumerate(m["sizes"]):  # what the gradient comparison needs: no tied column minimum
        cm = m["cost"][b, :nb, :nb] - m["u_pred"][b, :nb, None]
        assert ((cm == cm.min(axis=0)).sum(axis=0) == 1).all()
    bound = dl.reference_bounds(r, m["sizes"])
    assert (np.abs(m["ref_dual"] - r["dual64"]) <= bound["dual"]).all()
    assert (np.abs(m["ref_feas"] - r["feas64"]) <= bound["feas"]).all()
    assert (np.abs(m["ref_vreg"] - r["vreg64"]) <= bound["vreg"]).all()
    assert (np.abs(m["ref_grad"] - r["g64"]) <= bound["grad"]).all()
    assert (np.abs(m["ref_gvh"] - r["gvh64"]) <= bound["gvh"]).all()
    assert (r["vreg64"] > 0).all() and np.abs(r["gvh64"]).max() > 0
    for b, nb in enumerate(m["sizes"]):
        assert (m["ref_grad"][b, nb:] == 0).all() and (r["g64"][b, nb:] == 0).all()
        assert (m["ref_gvh"][b, nb:] == 0).all() and (r["gvh64"][b, nb:] == 0).all()


def test_v_reg_reaches_u_through_the_owning_row():
    """The sign and the routing of the second gradient of u, on two rows and three columns worked by hand: row 0
    owns columns 0 and 2, row 1 owns column 1."""
    C = np.array([[1.0, 5.0, 2.0], [4.0, 1.0, 6.0], [9.0, 9.0, 9.0]], dtype=np.float32)
    u = np.zeros(3, dtype=np.float32)
    vh = np.array([1.5, 0.0, 4.0], dtype=np.float32)
    r = dl.restate_instance(C, u, vh, 3, 1, weights=(0.0, 0.0, 1.0))
    assert r["a"].tolist() == [0, 1, 0] and r["v"].tolist() == [1.0, 1.0, 2.0]
    assert r["d"].tolist() == [0.5, -1.0, 2.0] and r["S"].tolist() == [2.5, -1.0, 0.0]
    assert np.allclose(r["g64"], [2 * 2.5 / 3, 2 * -1.0 / 3, 0.0]) and np.allclose(r["gvh64"], [1 / 3, -2 / 3, 4 / 3])
    assert r["vreg64"] == (0.25 + 1.0 + 4.0) / 3
    # a finite difference of v_reg in u_0 agrees: v_0 and v_2 fall as u_0 rises
    e = np.float32(2.0 ** -8)
    up = dl.restate_instance(C, u + np.array([e, 0, 0], np.float32), vh, 3, 1)["vreg64"]
    dn = dl.restate_instance(C, u - np.array([e, 0, 0], np.float32), vh, 3, 1)["vreg64"]
    assert abs((up - dn) / (2 * float(e)) - 2 * 2.5 / 3) < 1e-6


def test_integer_cases_are_tied():
    for k in ALL:
        m = CASES.case(k)
        if m["kind"] != "integer":
            continue
        tied = False
        for b, nb in enumerate(m["sizes"]):
            cm = m["cost"][b, :nb, :nb] - m["u_pred"][b, :nb, None]
            tied |= bool(((cm == cm.min(axis=0)).sum(axis=0) > 1).any())
        assert tied, LABELS[k]


def test_symbols_are_bound_declared_and_exported(lib):
    header = (ROOT / "include" / "lapwarm_hip.h").read_text()
    from lap import _hip
    for name in SYMBOLS:
        assert name in _hip.SIGNATURES, name
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m and len(m.group(1).split(",")) == len(_hip.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert "train.py:267-308" in header


def test_workspace_bytes(lib):
    for b, n in [(0, 33), (65536, 33), (2, 0), (2, 16385), (-1, 5), (5, -1)]:
        assert lib.lapwarm_dual_loss_workspace_bytes(b, n) == 0, (b, n)
    for b in acc.GRID_BATCH:
        for n in acc.GRID_N:
            one = lib.lapwarm_train_loss_workspace_bytes(b, n)
            dual = lib.lapwarm_dual_loss_workspace_bytes(b, n)
            # behind the slots of the OneGNN entries: d_j (float32) and S_i (float64), each rounded up to 256 bytes
            assert one > 0 and dual == one + -(-4 * b * n // 256) * 256 + -(-8 * b * n // 256) * 256, (b, n)
    golden = json.loads((ROOT / "tests" / "golden" / "abi_contract.json").read_text())
    points = [(b, n) for b in acc.GRID_BATCH + acc.OUT_BATCH for n in acc.GRID_N + acc.OUT_N]
    assert [lib.lapwarm_train_loss_workspace_bytes(b, n) for b, n in points] == golden["sizes"]["train_loss"]


def test_argument_codes_are_those_of_the_train_loss_entries(lib):
    """-2, -5 and -1 in the order of the train-loss entries, every call returning before the device sees a pointer."""
    golden = json.loads((ROOT / "tests" / "golden" / "abi_contract.json").read_text())["codes"]
    P = acc.P
    texts = []

    def ws_at(call):
        rc = call()
        texts.append(lib.lapwarm_last_error().decode())
        return rc

    fwd = acc._uniform(lib, "lapwarm_dual_loss_forward", "dual_loss",
                       lambda b, n, w, s: (P, b, n, P, P, P, P, P, P, P, P, w, s, None), ws_at, True)
    bwd = acc._uniform(lib, "lapwarm_dual_loss_backward", "dual_loss",
                       lambda b, n, w, s: (b, n, P, P, P, P, 1.0, P, P, w, s, None), ws_at, True)
    want = {"n=0": -2, "batch=0": -2, "n=16385": -5, "batch=65536": -2, "batch=65536,n=16385": -5, "n=16385,ws=0": -5,
            "ws short": -1}
    assert fwd == want and bwd == want
    assert fwd == golden["lapwarm_train_loss_forward"] and bwd == golden["lapwarm_train_loss_backward"]
    assert len(texts) == 2 and all(t.startswith("workspace too small") for t in texts)


def test_dual_warmstart_loss_rejects_bad_arguments_before_the_device(monkeypatch):
    import torch

    from gnn import losses
    from lap import _hip

    assert callable(losses.dual_warmstart_loss)
    assert list(inspect.signature(losses.dual_warmstart_loss).parameters) == ["cost", "u_pred", "v_hint", "mask", "weights"]
    assert inspect.signature(losses.dual_warmstart_loss).parameters["weights"].default == (1.0, 1.0, 0.1)
    assert "train.py:267-308" in losses.__doc__

    def no_device():
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_hip, "require_device", no_device)
    monkeypatch.setattr(_hip, "load", no_device)
    B, n = 2, 5
    cost = torch.zeros(B, n, n)
    u = torch.zeros(B, n)
    mask = torch.ones(B, n, dtype=torch.bool)
    f = losses.dual_warmstart_loss
    with pytest.raises(TypeError, match="v_hint and mask are required"):
        f(cost, u, None, mask)
    with pytest.raises(ValueError, match="weights"):
        f(cost, u, u, mask, weights=(1.0, 1.0))
    # types and dtypes in the order cost, u_pred, v_hint, mask; then shapes; then devices
    with pytest.raises(TypeError, match="cost must be torch.float32"):
        f(cost.double(), u.double(), u.double(), mask.float())
    with pytest.raises(TypeError, match="u_pred must be torch.float16 or torch.bfloat16 or torch.float32"):
        f(cost, u.double(), u.double(), mask.float())
    with pytest.raises(TypeError, match="v_hint must be torch.float16 or torch.bfloat16 or torch.float32"):
        f(cost, u, u.double(), mask.float())
    with pytest.raises(TypeError, match="mask must be torch.bool"):
        f(cost, u, u, mask.float())
    with pytest.raises(TypeError, match="Argument 'v_hint' must be a torch.Tensor"):
        f(cost, u, u.numpy(), mask)
    with pytest.raises(ValueError, match=r"cost must be \(B, n, n\)"):
        f(torch.zeros(B, n, n + 1), u, u, mask)
    with pytest.raises(ValueError, match=r"u_pred must be \(2, 5\)"):
        f(cost, torch.zeros(B, n + 1), torch.zeros(B, n + 1), mask)
    with pytest.raises(ValueError, match=r"v_hint must be \(2, 5\)"):
        f(cost, u, torch.zeros(B, n + 1), mask[:1])
    with pytest.raises(ValueError, match=r"mask must be \(2, 5\)"):
        f(cost, u, u, mask[:1])
    with pytest.raises(ValueError, match="must be on the GPU"):
        f(cost, u.bfloat16(), u.half(), mask)
    # the OneGNN loss checks as before
    with pytest.raises(TypeError, match="u_target must be torch.float32"):
        losses.warmstart_loss(cost, u, u.double(), mask)


def test_dual_training_batch_is_declared_beside_training_batch():
    from gnn.collate import DeviceBatch, DualDeviceBatch
    from gnn.pipeline import DualWarmStartPipeline, WarmStartPipeline
    names = [f.name for f in DualDeviceBatch.__dataclass_fields__.values()]
    assert names == ["cost", "u", "v", "row_feat", "col_feat", "edge_feat", "mask", "sizes"]
    assert [f.name for f in DeviceBatch.__dataclass_fields__.values()] == ["cost", "u", "v", "row_feat", "topk", "mask",
                                                                            "sizes"]
    p = inspect.signature(DualWarmStartPipeline.dual_training_batch).parameters
    assert list(p) == ["self", "costs", "dual_noise_std", "dual_noise_prob", "generator"]
    assert (p["dual_noise_std"].default, p["dual_noise_prob"].default, p["generator"].default) == (0.0, 0.0, None)
    assert list(inspect.signature(WarmStartPipeline.training_batch).parameters) == list(p)
    # (tests/test_dual_gnn_host.py pins predict_batch as the only method DualWarmStartPipeline defines itself: the
    # method lives beside training_batch and goes by the model's type, as the ragged prediction does)
    assert DualWarmStartPipeline.dual_training_batch is WarmStartPipeline.dual_training_batch
    assert "4096" in DualWarmStartPipeline.dual_training_batch.__doc__
    pipe = DualWarmStartPipeline.__new__(DualWarmStartPipeline)  # no device: the checks come first
    with pytest.raises(ValueError, match=r"dual_noise_prob must be in \[0, 1\], not -0.5"):
        pipe.dual_training_batch([np.zeros((2, 2))], dual_noise_std=0.1, dual_noise_prob=-0.5)
    with pytest.raises(TypeError, match="Argument 'generator' must be a torch.Generator"):
        pipe.dual_training_batch([np.zeros((2, 2))], dual_noise_std=0.1, dual_noise_prob=0.5, generator=3)
    import torch
    pipe.model = torch.nn.Linear(1, 1)
    with pytest.raises(TypeError, match="needs a pipeline around a DualGNN"):
        pipe.dual_training_batch([np.zeros((2, 2))])
