"""Writes tests/golden/prune_cases.npz: what the pruned exact solve (tests/prune_common.py, the NumPy restatement
of the contract) gives for the cases of prune_common.CASES when its sparse solve is the reference's lapmod_v.

    python tests/golden/make_prune.py          (from the repo root)

calls lapmod_v of oracle/_ref/liblapmod_ref.so (oracle.ref.lapmod_lib, as make_lapmod.py does) and the reference's
dense lapjv_internal (oracle.ref.dense_raw), and stores data only.  Per case: k, family, n, seed (the matrix is
prune_common.family_matrix(family, n, seed)), trace = the (nnz, viol) of every round, and the final x, v and cost.
Every case must be certified within max_rounds = 32, and its cost must equal the cost of the reference's dense
assignment exactly; both are asserted here.
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
sys.path.insert(0, str(HERE.parent))
from oracle import ref  # noqa: E402
import prune_common as pc  # noqa: E402


def main():
    lapmod = pc.reference_lapmod()
    assert lapmod is not None, "oracle/_ref/liblapmod_ref.so is needed"
    out = {"labels": np.array([c[0] for c in pc.CASES])}
    for label, family, n, k, seed in pc.CASES:
        C = pc.family_matrix(family, n, seed)
        res = pc.solve_pruned(C, k, lapmod, max_rounds=32)
        assert res["ret"] == 0 and res["viol_last"] == 0, (label, res["trace"])
        dret, dx, _ = ref.dense_raw(C)
        assert dret == 0 and pc.serial_cost(C, dx) == res["cost"], (label, pc.serial_cost(C, dx), res["cost"])
        if family != "constant" and family != "integer":
            assert np.array_equal(dx, res["x"]), label  # a unique optimum: the same assignment
        out[f"{label}__k"] = np.int64(k)
        out[f"{label}__family"] = np.array(family)
        out[f"{label}__n"] = np.int64(n)
        out[f"{label}__seed"] = np.int64(seed)
        out[f"{label}__trace"] = np.asarray(res["trace"], dtype=np.int64).reshape(-1, 2)
        out[f"{label}__x"] = res["x"].astype(np.int16)
        out[f"{label}__v"] = res["v"]
        out[f"{label}__cost"] = np.float64(res["cost"])
        print(f"{label}: rounds {res['rounds']}, nnz {res['nnz']} ({res['nnz'] / (n * n):.3f} of n^2), "
              f"trace {res['trace']}")
    path = HERE / "prune_cases.npz"
    np.savez_compressed(path, **out)
    print(f"{len(pc.CASES)} cases, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
