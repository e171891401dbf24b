"""Shared by test_dual_gnn_host.py and test_gpu_dual_gnn.py: the fixture reader, models built from the fixture's
weights, the bound for outputs compared against fp64, and the folded formulation written with torch ops."""
import numpy as np
import torch

from conftest import GOLDEN

ENTRIES = {"lapwarm_graph_features_workspace_bytes": 2, "lapwarm_graph_features_batched": 11,
           "lapwarm_dual_gnn_workspace_bytes": 3, "lapwarm_dual_edge_scores": 11, "lapwarm_dual_attention": 16}
ONEGNN_ABS = 1e-5  # what the project grants OneGNN against its CPU oracle: no bound here is looser

_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = np.load(GOLDEN / "dual_gnn_cases.npz", allow_pickle=False)
    return _cases


def cfg_labels():
    return [str(s) for s in cases()["cfg_labels"]]


def model_labels():
    return [str(s) for s in cases()["model_labels"]]


def feat_labels():
    return [str(s) for s in cases()["feat_labels"]]


def state_dict(cfg, dtype=torch.float32):
    z = cases()
    prefix = f"w/{cfg}/"
    return {k[len(prefix):]: torch.from_numpy(z[k]).to(dtype) for k in z.files if k.startswith(prefix)}


def build_model(cfg, dtype=torch.float32):
    from gnn.dual_gnn import DualGNN
    hidden, heads, layers, _ = (int(v) for v in cases()[f"cfg/{cfg}"])
    model = DualGNN(hidden_dim=hidden, layers=layers, heads=heads, dropout=0.1).to(dtype)
    model.load_state_dict(state_dict(cfg, dtype))
    return model.eval()


def model_inputs(label):
    """-> edge, row, col (float32 tensors with a batch axis), mask (bool tensor or None)"""
    z = cases()
    inp = label.split("@")[1]
    if inp == "pad":
        return (torch.from_numpy(z["pad/edge"]), torch.from_numpy(z["pad/row"]), torch.from_numpy(z["pad/col"]),
                torch.from_numpy(z["pad/mask"]))
    return tuple(torch.from_numpy(z[f"feat/{inp}/{k}"])[None] for k in ("edge", "row", "col")) + (None,)


def bound_from(dev):
    """4 x the fp32-against-fp64 deviation of the reference evaluation on the same case, and never looser than
    the 1e-5 absolute of OneGNN."""
    return min(4.0 * float(dev), ONEGNN_ABS)


def model_bound(label):
    """The bound of a model case, for u and for v_hint alike: 4 x the reference's own max|u32 - u64| on the case
    (`du` in the fixture).  The fixture also records dv = max|v32 - v64|, which is larger than du in most cases;
    it is printed for information and widens nothing."""
    return bound_from(cases()[f"out/{label}/du"])


def edge_scores_torch(edge, W1, b1, W2, b2, G):
    """scores (B, 2, H, N, N) = G . GELU(W2 GELU(W1 f + b1) + b2), in the dtype of the arguments."""
    gelu = torch.nn.functional.gelu
    h2 = gelu(gelu(edge @ W1.T + b1) @ W2.T + b2)       # (B, N, N, 128)
    s = torch.einsum("bijk,ok->boij", h2, G)
    B, _, N, _ = s.shape
    return s.reshape(B, 2, G.shape[0] // 2, N, N)


def attention_torch(scores, a_row, c_row, a_col, c_col, kbias, mask, row_val, col_val):
    """row_msg, col_msg (B, N, H * D) of lapwarm_dual_attention, in the dtype of the arguments."""
    B, _, H, N, _ = scores.shape
    D = row_val.shape[-1] // H
    keep = mask if mask is not None else torch.ones((B, N), dtype=torch.bool)
    pair = keep[:, None, :, None] & keep[:, None, None, :]

    def one(s, a, c, k, val):  # s (B, H, query, key)
        s = torch.nn.functional.leaky_relu(a[..., :, None] + c[..., None, :] + s + k[None, :, None, None], 0.2)
        s = s.masked_fill(~pair, float("-inf"))
        w = torch.softmax(s, dim=-1)
        w = torch.where(torch.isfinite(w), w, torch.zeros_like(w))
        out = torch.einsum("bhqk,bkhd->bqhd", w, val.reshape(B, N, H, D))
        return out.reshape(B, N, H * D)

    row_msg = one(scores[:, 0], a_row, c_row, kbias[:H], col_val)
    col_msg = one(scores[:, 1].transpose(-1, -2), a_col, c_col, kbias[H:], row_val)
    return row_msg, col_msg


def folded_forward(model, edge, row, col, mask):
    """The model's forward with every layer's messages computed from what DualLayer.folded_parameters hands to
    the kernels (a, c, G, k) by the two torch functions above: the fused path with torch ops in place of HIP."""
    with torch.no_grad():
        r, c = model.row_encoder(row), model.col_encoder(col)
        for layer in model.layers:
            f = layer.folded_parameters(layer.row_proj(r), layer.col_proj(c))
            lin1, lin2 = layer.edge_mlp[0], layer.edge_mlp[3]
            scores = edge_scores_torch(edge, lin1.weight, lin1.bias, lin2.weight, lin2.bias, f["G"])
            rm, cm = attention_torch(scores, f["a_row"], f["c_row"], f["a_col"], f["c_col"], f["kbias"], mask,
                                     layer.row_val(r), layer.col_val(c))
            r, c = layer._update(r, c, rm, cm)
        u = model.row_out(r).squeeze(-1)
        v = model.col_out(c).squeeze(-1)
        mean_u = u.mean(dim=-1, keepdim=True)
        u, v = u - mean_u, v + mean_u
        if mask is not None:
            u, v = u.masked_fill(~mask, 0.0), v.masked_fill(~mask, 0.0)
    return u, v
