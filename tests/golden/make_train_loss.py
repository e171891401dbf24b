#!/usr/bin/env python3
"""Generate tests/golden/train_loss_cases.npz and tests/golden/train_loss_large_ref.npz FROM THE REFERENCE.

Runs only where the reference repository exists (oracle/ref.py knows where).  It loads the reference's
gnn/train_one_gnn.py through oracle.ref.load_module (imported, never copied; an empty stand-in module answers its
`import h5py`, which only the dataset reader uses), calls its `compute_loss` on the CPU with
`u_pred.requires_grad_()` and stores data only:

  * the inputs: cost (B, n, n), u_pred, u_target (B, n) float32, sizes (B,);
  * the reference's per-instance v_proj, dual_lower, feas, u_reg, primal_upper (the locals of `compute_loss`
    when it returns) and its grad_u;
  * dual64, feas64, ureg64: the same sums over the same float32 terms in float64; g64: the closed-form gradient
    in float64 from the integer counts; the stable-order greedy's assign and primal_upper: all from
    tests/train_loss_common.py;
  * per case, whether the reference's primal_upper equals the stable-order one in every instance.  np.argsort's
    default sort is unstable and the reference always sorts ties, so this depends on the numpy build; the count
    is printed, not asserted.  (With numpy >= 2 the reference's `sum()` of float32 scalars also stays float32,
    where numpy 1.x promoted it to float64.)

The inputs come from the recipes of tests/train_loss_common.py (uniform_case, integer_case, sparse_inf_case),
which the GPU tests draw from as well.  train_loss_large_ref.npz holds no inputs: for the two n = 1028 cases of
tl.LARGE_REF_LABELS it stores the reference's v_proj, dual_lower, feas, u_reg and grad_u, the seed the inputs are
regenerated from and a CRC32 of their bytes.

It asserts that no valid column of a gradient case has two rows attaining its minimum (the reference's `min`
backward is unspecified there), and that the reference's float32 sums and grad_u lie within the recursive-summation
bound of the float64 values (train_loss_common.reference_bounds).

Usage:  python tests/golden/make_train_loss.py          (from the repo root)
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent / "train_loss_cases.npz"

sys.path[:0] = [str(ROOT / "tests"), str(ROOT)]
import train_loss_common as tl  # noqa: E402
from oracle.ref import load_module  # noqa: E402

OUT_LARGE = tl.LARGE_REF

ref = load_module("gnn/train_one_gnn.py", "_ref_train_one_gnn", stubs=("h5py",))

CAPTURED = ("v_proj", "dual_lower", "feas", "u_reg", "primal_upper")


def reference_loss(cost, u_pred, u_target, sizes):
    """compute_loss of the reference on the CPU: its per-instance locals and grad_u."""
    B, n = u_pred.shape
    mask = torch.arange(n)[None, :] < torch.from_numpy(sizes.astype(np.int64))[:, None]
    batch = ref.Batch(cost=torch.from_numpy(cost), u=torch.from_numpy(u_target), v=torch.zeros(B, n),
                      row_feat=torch.zeros(B, n, 1), mask=mask)
    u = torch.from_numpy(u_pred.copy()).requires_grad_()
    seen = {}

    def grab(frame, event, arg):
        if event == "return" and frame.f_code is ref.compute_loss.__code__:
            seen.update({k: frame.f_locals[k].detach().clone() for k in CAPTURED})

    sys.setprofile(grab)
    try:
        loss, _ = ref.compute_loss(batch, {"u": u})
    finally:
        sys.setprofile(None)
    loss.backward()
    out = {k: seen[k].numpy().astype(np.float32) for k in CAPTURED}
    out["grad_u"] = u.grad.numpy().astype(np.float32)
    return out


def check_against_restatement(label, m, got, r):
    """The assertions every gradient case has to pass: v bit-equal to the restatement, no tied column minimum,
    the reference's float32 sums and grad_u within the recursive-summation bound of the float64 values."""
    cost, u_pred, sizes = m["cost"], m["u_pred"], m["sizes"]
    assert tl.bits_equal32(got["v_proj"], r["v"]), label
    for b in range(len(sizes)):
        nb = int(sizes[b])
        cm = cost[b, :nb, :nb] - u_pred[b, :nb, None]
        assert ((cm == cm.min(axis=0)).sum(axis=0) == 1).all(), (label, b, "tied column minimum")
    bound = tl.reference_bounds(r, sizes)
    assert (np.abs(got["dual_lower"] - r["dual64"]) <= bound["dual"]).all(), label
    assert (np.abs(got["feas"] - r["feas64"]) <= bound["feas"]).all(), label
    assert (np.abs(got["u_reg"] - r["ureg64"]) <= bound["ureg"]).all(), label
    assert (np.abs(got["grad_u"] - r["g64"]) <= bound["grad"]).all(), label
    assert (r["feas64"][sizes > 2] > 0).all(), (label, "no positive hinge residue")


def write_large():
    """train_loss_large_ref.npz: recorded results of the reference for the cases of tl.LARGE_REF_LABELS, whose
    inputs tl.large_case() regenerates; primal_upper is left out (it depends on an unstable sort)."""
    arrays, meta = {}, []
    for k, label in enumerate(tl.LARGE_REF_LABELS):
        m = tl.large_case(label)
        got = reference_loss(m["cost"], m["u_pred"], m["u_target"], m["sizes"])
        r = tl.restate(m["cost"], m["u_pred"], m["u_target"], m["sizes"])
        check_against_restatement(label, m, got, r)
        meta.append(dict(label=label, kind=m["kind"], B=m["B"], n=m["n"], seed=m["seed"], crc=tl.input_crc(m)))
        store = dict(ref_v=got["v_proj"], ref_dual=got["dual_lower"], ref_feas=got["feas"], ref_ureg=got["u_reg"],
                     ref_grad=got["grad_u"])
        arrays.update({f"c{k}_{name}": a for name, a in store.items()})
    np.savez_compressed(OUT_LARGE, meta=np.array(json.dumps(meta)), **arrays)
    print(f"{OUT_LARGE.name}: {len(meta)} cases, {OUT_LARGE.stat().st_size} bytes")


def main():
    rng = np.random.default_rng(20240611)
    specs = []
    for n in (1, 2, 7, 63, 64, 65, 257):
        for B in (1, 3):
            specs.append(("uniform", f"uniform-n{n}-B{B}", B, n, [n] * B))
    specs.append(("uniform", "uniform-n65-mixed", 4, 65, [65, 64, 1, 33]))
    for n in (2, 7, 64, 65):
        specs.append(("integer", f"integer-n{n}-B3", 3, n, [n] * 3))
    specs.append(("integer", "integer-n65-mixed", 4, 65, [65, 64, 1, 33]))

    arrays, meta, agree = {}, [], 0
    for k, (kind, label, B, n, sizes) in enumerate(specs):
        sizes = np.asarray(sizes, dtype=np.int32)
        cost, u_pred, u_target = tl.RECIPES[kind](rng, B, n, sizes)
        got = reference_loss(cost, u_pred, u_target, sizes)
        r = tl.restate(cost, u_pred, u_target, sizes)
        assert tl.bits_equal32(got["v_proj"], r["v"]), label
        if kind == "uniform":
            check_against_restatement(label, dict(cost=cost, u_pred=u_pred, sizes=sizes), got, r)
        primal_equal = bool(tl.bits_equal32(got["primal_upper"], r["primal_upper"]))
        agree += primal_equal
        meta.append(dict(label=label, kind=kind, B=B, n=n, primal_equal=primal_equal))
        store = dict(cost=cost, u_pred=u_pred, u_target=u_target, sizes=sizes, ref_v=got["v_proj"],
                     ref_dual=got["dual_lower"], ref_feas=got["feas"], ref_ureg=got["u_reg"],
                     ref_primal=got["primal_upper"], ref_grad=got["grad_u"], dual64=r["dual64"], feas64=r["feas64"],
                     ureg64=r["ureg64"], g64=r["g64"], assign=r["assign"], primal_stable=r["primal_upper"])
        if kind == "uniform" and n >= 257:
            store["cost_q"] = tl.grid_from_cost(store.pop("cost"))
        arrays.update({f"c{k}_{name}": a for name, a in store.items()})
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **arrays)
    print(f"{OUT.name}: {len(meta)} cases, {OUT.stat().st_size} bytes; reference primal_upper equals the "
          f"stable-order one in {agree} of {len(meta)} cases (numpy {np.__version__})")


if __name__ == "__main__":
    main()
    write_large()
