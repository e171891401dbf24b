"""Writes tests/golden/dual_gnn_cases.npz: the reference's graph features and DualGNN outputs.

Runs only where the reference repository exists (oracle/ref.py knows where).  It loads the reference's
gnn/features.py and gnn/dual_gnn.py through oracle.ref.load_module (in a stand-in package named _ref_gnn, so that
the model's relative import of the features resolves) and never copies them.

Usage:  python tests/golden/make_dual_gnn.py          (from the repo root)

Feature cases (`feat_labels`): cost C, the reference's edge_feat, row_feat, col_feat, and u where the case has one.
Model configurations (`cfg_labels`): seeded random weights, stored as arrays `w/<cfg>/<parameter name>`.  The
weights are rounded to multiples of 2^-10 so that the compressed file stays small; they are ordinary float32
arrays and the reference is evaluated on exactly these values.
Model cases (`model_labels`): configuration, inputs (a feature case, or the padded batch `pad/*`), the reference's
eval-mode u and v_hint in float32 (u32, v32) and from a .double() copy of the same weights and inputs (u64, v64),
and the reference's own float32 deviations du = max|u32 - u64| and dv = max|v32 - v64|, each on its own: the tests
bound both outputs by 4 x du; dv is recorded for information.
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from oracle.ref import load_module  # noqa: E402

OUT = Path(__file__).resolve().parent / "dual_gnn_cases.npz"

CONFIGS = {"h32_H4_L2": (32, 4, 2), "h128_H4_L1": (128, 4, 1), "h64_H8_L1": (64, 8, 1)}
PARAM_COUNTS = {"h32_H4_L2": 62418, "h128_H4_L1": 171658}
PAD_SIZES = (40, 33, 1)


def feature_cases(rf):
    rng = np.random.default_rng(20261019)
    cases = {}
    for n in (1, 2, 3, 17, 64, 65):
        cases[f"uniform_n{n}"] = (rng.random((n, n)), None)
    cases["reduced_n17"] = (rng.random((17, 17)) * 5.0, rng.random(17) * 2.0 - 1.0)
    cases["ties_int_n40"] = (np.floor(rng.random((40, 40)) * 8.0), None)
    C = rng.random((9, 9)) * 3.0
    C[4, :] = 1.25
    cases["const_row_n9"] = (C, None)
    out = {}
    for label, (C, u) in cases.items():
        f = rf.compute_features(C, include_reduced_cost=u is not None, u=u)
        out[label] = dict(C=C, u=u, edge=f.edge_feat, row=f.row_feat, col=f.col_feat)
    return out


def seeded_model(rm, hidden, heads, layers, seed):
    torch.manual_seed(seed)
    model = rm.DualGNN(hidden_dim=hidden, layers=layers, heads=heads, dropout=0.1)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.ndim == 1:  # biases and LayerNorm: away from their 0 / 1 defaults
                p.add_(torch.empty_like(p).uniform_(-0.1, 0.1, generator=g))
            p.copy_(torch.round(p * 1024.0) / 1024.0)
    return model.eval()


def run(model, edge, row, col, mask):
    with torch.no_grad():
        o32 = model(edge, row, col, mask)
        m64 = type(model)(hidden_dim=model.hidden_dim, layers=len(model.layers), heads=model.heads).double().eval()
        m64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
        o64 = m64(edge.double(), row.double(), col.double(), mask)
    return o32["u"].numpy(), o32["v_hint"].numpy(), o64["u"].numpy(), o64["v_hint"].numpy()


def main():
    rf = load_module("gnn/features.py", "features", package="_ref_gnn")
    rm = load_module("gnn/dual_gnn.py", "dual_gnn", package="_ref_gnn")
    feats = feature_cases(rf)
    z = {"feat_labels": np.array(list(feats))}
    for label, f in feats.items():
        z[f"feat/{label}/C"] = f["C"]
        z[f"feat/{label}/edge"], z[f"feat/{label}/row"], z[f"feat/{label}/col"] = f["edge"], f["row"], f["col"]
        if f["u"] is not None:
            z[f"feat/{label}/u"] = f["u"]

    # the padded batch: every instance's features at its own size, zero-padded to N
    rng = np.random.default_rng(7)
    N = max(PAD_SIZES)
    pad_edge = np.zeros((len(PAD_SIZES), N, N, rf.EDGE_FEATURE_DIM), np.float32)
    pad_row = np.zeros((len(PAD_SIZES), N, rf.NODE_FEATURE_DIM), np.float32)
    pad_col = np.zeros_like(pad_row)
    pad_mask = np.zeros((len(PAD_SIZES), N), bool)
    for b, n in enumerate(PAD_SIZES):
        f = rf.compute_features(rng.random((n, n)) * 10.0)
        pad_edge[b, :n, :n], pad_row[b, :n], pad_col[b, :n], pad_mask[b, :n] = f.edge_feat, f.row_feat, f.col_feat, True
    z["pad/edge"], z["pad/row"], z["pad/col"], z["pad/mask"] = pad_edge, pad_row, pad_col, pad_mask
    z["pad/sizes"] = np.array(PAD_SIZES)

    inputs = {k: (feats[k]["edge"][None], feats[k]["row"][None], feats[k]["col"][None], None)
              for k in ("uniform_n17", "uniform_n64", "uniform_n65")}
    inputs["pad"] = (pad_edge, pad_row, pad_col, pad_mask)
    model_labels = []
    for c, (cfg, (hidden, heads, layers)) in enumerate(CONFIGS.items()):
        model = seeded_model(rm, hidden, heads, layers, 100 + c)
        count = sum(p.numel() for p in model.parameters())
        assert PARAM_COUNTS.get(cfg, count) == count, (cfg, count)
        z[f"cfg/{cfg}"] = np.array([hidden, heads, layers, count])
        for name, v in model.state_dict().items():
            z[f"w/{cfg}/{name}"] = v.numpy()
        for inp, (edge, row, col, mask) in inputs.items():
            t = [torch.from_numpy(a) for a in (edge, row, col)]
            u32, v32, u64, v64 = run(model, *t, None if mask is None else torch.from_numpy(mask))
            label = f"{cfg}@{inp}"
            model_labels.append(label)
            z[f"out/{label}/u32"], z[f"out/{label}/v32"] = u32, v32
            z[f"out/{label}/u64"], z[f"out/{label}/v64"] = u64, v64
            du, dv = np.abs(u32 - u64).max(), np.abs(v32 - v64).max()
            z[f"out/{label}/du"], z[f"out/{label}/dv"] = np.array(du), np.array(dv)
            print(f"{label}: reference fp32 against fp64 u {du:.3e}, v_hint {dv:.3e}, max|u| {np.abs(u64).max():.3f}")
    z["cfg_labels"] = np.array(list(CONFIGS))
    z["model_labels"] = np.array(model_labels)
    np.savez_compressed(OUT, **z)
    print(f"{OUT.name}: {OUT.stat().st_size} bytes")
    assert OUT.stat().st_size <= 1 << 20


if __name__ == "__main__":
    main()
