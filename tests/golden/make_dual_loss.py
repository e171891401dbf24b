#!/usr/bin/env python3
"""Generate tests/golden/dual_loss_cases.npz FROM THE REFERENCE.

Runs only where the reference repository exists (oracle/ref.py knows where).  It loads the reference's gnn/train.py
through oracle.ref.load_module (imported, never copied).  An empty stand-in module answers its `import h5py`, which
only the dataset reader uses; its `from gnn import DualGNN, compute_features, EDGE_FEATURE_DIM, NODE_FEATURE_DIM` is
answered by a stand-in module `gnn` that holds those four names of the reference's own gnn/dual_gnn.py and
gnn/features.py, loaded the same way, and is taken out of sys.modules again.  It calls the reference's `compute_loss`
on the CPU with `u_pred.requires_grad_()` and `v_hint.requires_grad_()` and stores data only:

  * the inputs: cost (B, n, n), u_pred, v_hint (B, n) float32, sizes (B,); from n = 257 the costs as the 12-bit
    integers of train_loss_common.cost_from_grid;
  * the reference's per-instance v_proj, dual_lower, feas, v_reg, primal_upper (the locals of `compute_loss` when it
    returns) and its gradients for u_pred and v_hint;
  * per case, whether the reference's primal_upper equals the stable-order one in every instance (np.argsort's
    default sort is unstable: printed, not asserted).

The inputs come from the recipes of tests/train_loss_common.py; v_hint takes the place of u_target.

In the cases whose gradient is compared with autograd (the uniform ones) it asserts that no column minimum is tied:
torch's `min` backward would otherwise decide grad_u.  Row minima of the reduced costs are ALWAYS tied as soon as a
row attains two column minima (its reduced cost is exactly 0 at both), which a random instance of n = 33 or more
always has; they reach only the greedy's row order and so primal_upper, a constant for autograd, never a gradient.
The generator therefore records `rows_untied` per case instead of asserting it, and the tests compare primal_upper
with the reference only where `primal_equal` says the unstable sort happened to agree.  It also asserts that the
reference's float32 sums and gradients lie within dual_loss_common.reference_bounds of the float64 restatement.

Usage:  python tests/golden/make_dual_loss.py          (from the repo root)
"""
from __future__ import annotations

import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]

sys.path[:0] = [str(ROOT / "tests"), str(ROOT)]
import dual_loss_common as dl  # noqa: E402
import train_loss_common as tl  # noqa: E402
from oracle.ref import load_module  # noqa: E402

OUT = dl.GOLDEN
CAPTURED = ("v_proj", "dual_lower", "feas", "v_reg", "primal_upper")


def load_reference_train():
    rf = load_module("gnn/features.py", "features", package="_ref_gnn")
    rm = load_module("gnn/dual_gnn.py", "dual_gnn", package="_ref_gnn")
    stand_in = types.ModuleType("gnn")
    stand_in.DualGNN, stand_in.compute_features = rm.DualGNN, rf.compute_features
    stand_in.EDGE_FEATURE_DIM, stand_in.NODE_FEATURE_DIM = rf.EDGE_FEATURE_DIM, rf.NODE_FEATURE_DIM
    before = sys.modules.get("gnn")
    sys.modules["gnn"] = stand_in
    try:
        return load_module("gnn/train.py", "_ref_train", stubs=("h5py",))
    finally:
        if before is None:
            del sys.modules["gnn"]
        else:
            sys.modules["gnn"] = before


ref = load_reference_train()


def reference_loss(cost, u_pred, v_hint, sizes):
    """compute_loss of the reference on the CPU: its per-instance locals and the two gradients."""
    B, n = u_pred.shape
    mask = torch.arange(n)[None, :] < torch.from_numpy(sizes.astype(np.int64))[:, None]
    zero = torch.zeros(B, n)
    batch = ref.Batch(cost=torch.from_numpy(cost), u=zero, v=zero, row_feat=torch.zeros(B, n, 1),
                      col_feat=torch.zeros(B, n, 1), edge_feat=torch.zeros(B, n, n, 1), mask=mask)
    u = torch.from_numpy(u_pred.copy()).requires_grad_()
    vh = torch.from_numpy(v_hint.copy()).requires_grad_()
    seen = {}

    def grab(frame, event, arg):
        if event == "return" and frame.f_code is ref.compute_loss.__code__:
            seen.update({k: frame.f_locals[k].detach().clone() for k in CAPTURED})

    sys.setprofile(grab)
    try:
        loss, _ = ref.compute_loss(batch, {"u": u, "v_hint": vh})
    finally:
        sys.setprofile(None)
    loss.backward()
    out = {k: seen[k].numpy().astype(np.float32) for k in CAPTURED}
    out["grad_u"] = u.grad.numpy().astype(np.float32)
    out["grad_vh"] = vh.grad.numpy().astype(np.float32)
    return out


def check_against_restatement(label, cost, u_pred, sizes, got, r):
    assert tl.bits_equal32(got["v_proj"], r["v"]), label
    for b in range(len(sizes)):
        nb = int(sizes[b])
        cm = cost[b, :nb, :nb] - u_pred[b, :nb, None]
        assert ((cm == cm.min(axis=0)).sum(axis=0) == 1).all(), (label, b, "tied column minimum")
    bound = dl.reference_bounds(r, sizes)
    assert (np.abs(got["dual_lower"] - r["dual64"]) <= bound["dual"]).all(), label
    assert (np.abs(got["feas"] - r["feas64"]) <= bound["feas"]).all(), label
    assert (np.abs(got["v_reg"] - r["vreg64"]) <= bound["vreg"]).all(), label
    assert (np.abs(got["grad_u"] - r["g64"]) <= bound["grad"]).all(), label
    assert (np.abs(got["grad_vh"] - r["gvh64"]) <= bound["gvh"]).all(), label


def main():
    rng = np.random.default_rng(20250917)
    specs = [("uniform", f"uniform-n{n}-B2", 2, n, [n] * 2) for n in (1, 5, 33, 64)]
    specs.append(("uniform", "uniform-n257-B1", 1, 257, [257]))
    specs.append(("uniform", "uniform-n64-mixed", 4, 64, [64, 33, 1, 5]))
    specs.append(("uniform", "uniform-n257-mixed", 2, 257, [257, 130]))
    specs.append(("integer", "integer-n5-B3", 3, 5, [5] * 3))
    specs.append(("integer", "integer-n33-B3", 3, 33, [33] * 3))
    specs.append(("integer", "integer-n64-mixed", 4, 64, [64, 33, 1, 5]))

    arrays, meta, agree = {}, [], 0
    for k, (kind, label, B, n, sizes) in enumerate(specs):
        sizes = np.asarray(sizes, dtype=np.int32)
        cost, u_pred, v_hint = tl.RECIPES[kind](rng, B, n, sizes)
        if kind == "uniform" and n >= 257:  # the padding on the grid as well: finite rubbish that q can store
            rubbish = tl.cost_from_grid(np.uint16(4095))
            for b, nb in enumerate(sizes):
                cost[b, nb:, :] = rubbish
                cost[b, :, nb:] = rubbish
        got = reference_loss(cost, u_pred, v_hint, sizes)
        r = dl.restate(cost, u_pred, v_hint, sizes)
        assert tl.bits_equal32(got["v_proj"], r["v"]), label
        if kind == "uniform":
            check_against_restatement(label, cost, u_pred, sizes, got, r)
        primal_equal = bool(tl.bits_equal32(got["primal_upper"], r["primal_upper"]))
        agree += primal_equal
        meta.append(dict(label=label, kind=kind, B=B, n=n, primal_equal=primal_equal,
                         rows_untied=bool(dl.untied(cost, u_pred, r["v"], sizes))))
        store = dict(cost=cost, u_pred=u_pred, v_hint=v_hint, sizes=sizes, ref_v=got["v_proj"],
                     ref_dual=got["dual_lower"], ref_feas=got["feas"], ref_vreg=got["v_reg"],
                     ref_primal=got["primal_upper"], ref_grad=got["grad_u"], ref_gvh=got["grad_vh"])
        if kind == "uniform" and n >= 257:
            store["cost_q"] = tl.grid_from_cost(store.pop("cost"))
        arrays.update({f"c{k}_{name}": a for name, a in store.items()})
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **arrays)
    print(f"{OUT.name}: {len(meta)} cases, {OUT.stat().st_size} bytes; reference primal_upper equals the "
          f"stable-order one in {agree} of {len(meta)} cases (numpy {np.__version__})")


if __name__ == "__main__":
    main()
