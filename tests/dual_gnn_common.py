"""Shared by test_dual_gnn_host.py and the GPU tests of DualGNN: the fixture reader, models built from the fixture's
weights, the bound for outputs compared against fp64, the folded formulation written with torch ops, and the graph
features in NumPy fp64 with stable ranks."""
import numpy as np
import torch

from conftest import GOLDEN

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


# ---- the graph features in NumPy ------------------------------------------------------------------------------

FEATURE_EPS = 1e-9   # added to both entropy terms; the floor of the MAD
FEATURE_TAU = 1e-3   # a gap up to this counts as a tie with the minimum


def _side_numpy(C, axis):
    """The statistics of every line of C along `axis` (1: rows, 0: columns), each with that axis kept at length 1:
    min, max, mean, population std, median, MAD floored at FEATURE_EPS, entropy, tie share, and the stable ranks
    0..n-1 (the lower index first among equal values) as an (n, n) integer array."""
    n = C.shape[axis]
    s = {"min": C.min(axis=axis, keepdims=True), "max": C.max(axis=axis, keepdims=True),
         "mean": C.mean(axis=axis, keepdims=True), "std": C.std(axis=axis, keepdims=True),
         "med": np.median(C, axis=axis, keepdims=True)}
    mad = np.median(np.abs(C - s["med"]), axis=axis, keepdims=True)
    s["mad"] = np.where(mad < FEATURE_EPS, FEATURE_EPS, mad)
    p = np.exp(-C)  # not stabilised: exp(-C) as it is
    p = p / (p.sum(axis=axis, keepdims=True) + FEATURE_EPS)
    s["ent"] = -(p * np.log(p + FEATURE_EPS)).sum(axis=axis, keepdims=True)
    s["gap"] = C - s["min"]
    s["tie"] = (s["gap"] <= FEATURE_TAU).sum(axis=axis, keepdims=True) / max(1, n)
    order = np.argsort(C, axis=axis, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(n).reshape((1, n) if axis == 1 else (n, 1)), axis=axis)
    s["rank"] = rank
    return s


def _features_numpy_one(C, u):
    from gnn.features import positional_encodings
    n = C.shape[0]
    r, c = _side_numpy(C, 1), _side_numpy(C, 0)
    full = lambda a: np.broadcast_to(a, (n, n))  # noqa: E731
    d = max(1, n - 1)
    if u is None:
        reduced = np.zeros((n, n))
    else:
        lifted = C - u[:, None]
        reduced = lifted - lifted.min(axis=0, keepdims=True)
    edge = np.stack([(C - r["med"]) / r["mad"], r["rank"] / d, c["rank"] / d, r["gap"], c["gap"], full(r["tie"]),
                     full(c["tie"]), full(r["ent"]), full(c["ent"]), reduced], axis=-1).astype(np.float32)
    pos = positional_encodings(n)
    node = lambda s: np.concatenate(  # noqa: E731
        [s[k].reshape(n, 1) for k in ("min", "max", "mean", "std", "mad", "ent")] + [pos], axis=1).astype(np.float32)
    return edge, node(r), node(c)


def features_numpy(C, u=None):
    """The graph features of graph_features_device in NumPy fp64, rounded once to float32: C (n, n) or (B, n, n),
    u (n,), (B, n) or None -> edge (.., n, n, 10), row (.., n, 14), col (.., n, 14).  Edge channels: the cost scaled
    by the row's median and MAD, row rank, column rank (stable, over max(1, n - 1)), gap to the row minimum, gap to
    the column minimum, tie share of the row, of the column, entropy of the row, of the column, and
    C - u - min_i(C - u) (0 without u).  Node channels: min, max, mean, std, MAD, entropy, 8 positional encodings."""
    C = np.asarray(C, dtype=np.float64)
    if C.ndim == 2:
        return _features_numpy_one(C, None if u is None else np.asarray(u, dtype=np.float64).reshape(-1))
    us = [None] * C.shape[0] if u is None else np.asarray(u, dtype=np.float64).reshape(C.shape[0], -1)
    parts = [_features_numpy_one(Cb, ub) for Cb, ub in zip(C, us)]
    return tuple(np.stack(p) for p in zip(*parts))


def assert_valid_stable_ranks(values, ranks):
    """each row of `ranks` is a permutation of 0..n-1, non-decreasing in the value, increasing in the index among
    equal values"""
    n = values.shape[1]
    for i in range(values.shape[0]):
        r = ranks[i]
        assert sorted(r.tolist()) == list(range(n)), i
        order = np.argsort(r)
        v = values[i][order]
        assert np.all(np.diff(v) >= 0), i
        same = np.diff(v) == 0
        assert np.all(np.diff(order)[same] > 0), i


def integer_ranks(channel, n):
    """The ranks 0..n-1 behind a float32 rank channel, after checking that every entry is exactly k / max(1, n - 1)
    rounded to float32."""
    d = max(1, n - 1)
    k = np.rint(channel.astype(np.float64) * d).astype(np.int64)
    assert np.array_equal((k / d).astype(np.float32), channel)
    return k
