"""References for the backward of DualGNN's fused attention (csrc/dual_gnn.hip: lapwarm_dual_attention_backward,
lapwarm_dual_edge_scores_backward) -- TEST INFRASTRUCTURE, no GPU needed.

`attention_backward_ref` and `edge_scores_backward_ref` restate the closed forms of include/lapwarm_hip.h in fp64;
`attention_autograd` and `edge_scores_autograd` are torch autograd through dual_gnn_common.attention_torch /
edge_scores_torch in a dtype of the caller's choice: float64 is the reference of the kernel tests, float32 on the
CPU the yardstick of refine_backward_common.tolerance."""
import math

import numpy as np
import torch

import dual_gnn_common as dg

ATT_NAMES = ("dS", "da_row", "dc_row", "da_col", "dc_col", "dkb", "d_row_val", "d_col_val")
EDGE_NAMES = ("dW1", "db1", "dW2", "db2", "dG")


# ---- inputs ----------------------------------------------------------------------------------------------------

def attention_case(B, N, H, D, mask_kind="none", scale=1.0, seed=0, sizes=None):
    """float32 CPU tensors: the nine forward arguments of dg.attention_torch (mask: bool (B, N) or None) and the two
    message gradients.  mask_kind: none | prefix | scattered | one_empty (instance 0 fully masked).  `sizes`: the
    sizes of the prefix mask in place of prefix_sizes(B, N); one outside 1..N is an empty instance."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * N + 31 * H + D)
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    scores = r(B, 2, H, N, N) * scale
    a_row, c_row, a_col, c_col = (r(B, H, N) * scale for _ in range(4))
    kbias = r(2 * H) * 0.5 * scale
    row_val, col_val = r(B, N, H * D), r(B, N, H * D)
    if mask_kind == "none":
        mask = None
    elif mask_kind == "prefix":
        mask = prefix_mask(prefix_sizes(B, N) if sizes is None else sizes, N)
    elif mask_kind == "scattered":
        mask = torch.rand((B, N), generator=g) < 0.6
        mask[:, N // 2] = True
    elif mask_kind == "one_empty":
        mask = torch.rand((B, N), generator=g) < 0.7
        mask[:, 0] = True
        mask[0] = False
    else:
        raise ValueError(mask_kind)
    return (scores, a_row, c_row, a_col, c_col, kbias, mask, row_val, col_val), (r(B, N, H * D), r(B, N, H * D))


def prefix_sizes(B, N):
    """sizes (B,) int64 in 1..N, the first N itself when B > 1, the others spread below it."""
    return torch.tensor([N if (b == 0 and B > 1) else max(1, (N * (b + 2)) // (B + 2)) for b in range(B)])


def prefix_mask(sizes, N):
    """bool (B, N): node i of instance b is real when i < sizes[b]; a size outside 1..N is an empty instance."""
    sizes = torch.as_tensor(sizes, dtype=torch.int64)
    inside = (sizes >= 1) & (sizes <= N)
    return torch.arange(N)[None, :] < torch.where(inside, sizes, torch.zeros_like(sizes))[:, None]


# ---- the wave tiles of the edge backward -------------------------------------------------------------------------
# With sizes lapwarm_dual_edge_scores_backward walks the edges (i, j < sizes[b]) only, a wave tile of 16 at a time as
# lapwarm_dual_edge_scores_ragged numbers them: instance after instance, row after row, 16 columns at a time, so
# n * ceil(n / 16) tiles for a size in 1..N and none for any other ("an empty instance", include/lapwarm_hip.h).
# Without sizes a tile is 16 edges of the linear order.  A chunk is lapwarm_dual_backward_chunk() / 16 tiles.

WAVE_EDGES = 16


def ragged_wave_tiles(sizes, N):
    """The number of wave tiles of every instance in the ragged numbering."""
    return [n * -(-n // WAVE_EDGES) if 1 <= n <= N else 0 for n in (int(s) for s in sizes)]


def chunk_crossings(sizes, N, chunk):
    """[(t0, b, offset)] for every chunk start t0 > 0 (in wave tiles, `chunk` in edges) below the total of the
    ragged numbering: the instance whose tiles contain t0 and the tile's number inside it.  offset 0: the chunk
    starts with the instance."""
    per = chunk // WAVE_EDGES
    counts = ragged_wave_tiles(sizes, N)
    out = []
    for t0 in range(per, sum(counts), per):
        first = 0
        for b, count in enumerate(counts):
            if first <= t0 < first + count:
                out.append((t0, b, t0 - first))
                break
            first += count
    return out


def ragged_tile_edges(sizes, N, t):
    """[(b, i, j)]: the edges of wave tile t of the ragged numbering, the columns past the size left out."""
    first = 0
    for b, count in enumerate(ragged_wave_tiles(sizes, N)):
        if first <= t < first + count:
            n = int(sizes[b])
            groups = -(-n // WAVE_EDGES)
            i, g = divmod(t - first, groups)
            return [(b, i, j) for j in range(g * WAVE_EDGES, min(n, (g + 1) * WAVE_EDGES))]
        first += count
    raise ValueError(f"tile {t} is past the {first} tiles of the sizes")


def uniform_tile_edges(B, N, t):
    """[(b, i, j)]: the edges of wave tile t of the uniform numbering, 16 at a time in the linear edge order."""
    return [(e // (N * N), e // N % N, e % N) for e in range(t * WAVE_EDGES, min(B * N * N, (t + 1) * WAVE_EDGES))]


def probe_gradient(dS, edges):
    """dS with zeros everywhere but on `edges` [(b, i, j)], every output channel of those kept."""
    out = torch.zeros_like(dS)
    for b, i, j in edges:
        out[b, :, :, i, j] = dS[b, :, :, i, j]
    return out


def edge_case(B, N, heads, seed=0):
    """float32 CPU tensors (edge, W1, b1, W2, b2, G) in the ranges of the forward's tests, and dS (B, 2, heads, N, N)."""
    g = torch.Generator().manual_seed(7919 * seed + 1000 * N + heads + 17 * B)
    edge = torch.rand((B, N, N, 10), generator=g) * 2.0 - 0.5
    W1 = (torch.rand((128, 10), generator=g) - 0.5) * 0.6
    b1 = (torch.rand((128,), generator=g) - 0.5) * 0.2
    W2 = (torch.rand((128, 128), generator=g) - 0.5) * 0.18
    b2 = (torch.rand((128,), generator=g) - 0.5) * 0.2
    G = (torch.rand((2 * heads, 128), generator=g) - 0.5) * 0.3
    dS = torch.randn((B, 2, heads, N, N), generator=g)
    return (edge, W1, b1, W2, b2, G), dS


# ---- autograd --------------------------------------------------------------------------------------------------

def attention_autograd(args, grads, dtype=torch.float64):
    """dict of ATT_NAMES -> tensors of `dtype`: autograd of sum(row_msg * g_row) + sum(col_msg * g_col) through
    dg.attention_torch.  dkb is (2 H,)."""
    scores, a_row, c_row, a_col, c_col, kbias, mask, row_val, col_val = args
    leaves = [t.detach().to(dtype).requires_grad_() for t in (scores, a_row, c_row, a_col, c_col, kbias, row_val, col_val)]
    s, ar, cr, ac, cc, kb, rv, cv = leaves
    rm, cm = dg.attention_torch(s, ar, cr, ac, cc, kb, mask, rv, cv)
    ((rm * grads[0].to(dtype)).sum() + (cm * grads[1].to(dtype)).sum()).backward()
    return dict(zip(ATT_NAMES, (t.grad for t in leaves)))


def edge_scores_autograd(args, dS, dtype=torch.float64):
    """dict of EDGE_NAMES: autograd of sum(scores * dS) through dg.edge_scores_torch; no gradient for the features."""
    edge = args[0].detach().to(dtype)
    leaves = [t.detach().to(dtype).requires_grad_() for t in args[1:]]
    (dg.edge_scores_torch(edge, *leaves) * dS.to(dtype)).sum().backward()
    return dict(zip(EDGE_NAMES, (t.grad for t in leaves)))


# ---- the closed forms of the header, fp64 ----------------------------------------------------------------------

def attention_backward_ref(args, grads):
    """The closed form of lapwarm_dual_attention_backward in fp64 NumPy: dict of ATT_NAMES -> arrays."""
    scores, a_row, c_row, a_col, c_col, kbias, mask, row_val, col_val = (
        None if t is None else t.detach().numpy().astype(np.float64 if t.dtype != torch.bool else bool) for t in args)
    B, _, H, N, _ = scores.shape
    D = row_val.shape[-1] // H
    keep = np.ones((B, N), bool) if mask is None else mask
    pair = keep[:, None, :, None] & keep[:, None, None, :]

    def one(S, a, c, kb, val, dmsg):  # S (B, H, query, key); val, dmsg (B, N, H, D)
        z = a[..., :, None] + c[..., None, :] + S + kb[None, :, None, None]
        s = np.where(z >= 0, z, 0.2 * z)
        s = np.where(pair, s, -np.inf)
        m = s.max(axis=-1, keepdims=True)
        e = np.where(pair, np.exp(s - np.where(np.isfinite(m), m, 0.0)), 0.0)
        tot = e.sum(axis=-1, keepdims=True)
        w = np.where(tot > 0, e / np.where(tot > 0, tot, 1.0), 0.0)
        msg = np.einsum("bhqk,bkhd->bqhd", w, val)
        delta = np.einsum("bqhd,bqhd->bhq", dmsg, msg)
        dw = np.einsum("bqhd,bkhd->bhqk", dmsg, val)
        dz = np.where(pair, w * (dw - delta[..., None]) * np.where(z >= 0, 1.0, 0.2), 0.0)
        return dz, dz.sum(-1), dz.sum(-2), dz.sum((0, 2, 3)), np.einsum("bhqk,bqhd->bkhd", w, dmsg).reshape(B, N, H * D)

    g_row, g_col = (g.detach().numpy().astype(np.float64).reshape(B, N, H, D) for g in grads)
    rv, cv = row_val.reshape(B, N, H, D), col_val.reshape(B, N, H, D)
    dz0, da0, dc0, dk0, d_col_val = one(scores[:, 0], a_row, c_row, kbias[:H], cv, g_row)
    dz1, da1, dc1, dk1, d_row_val = one(scores[:, 1].swapaxes(-1, -2), a_col, c_col, kbias[H:], rv, g_col)
    dS = np.stack([dz0, dz1.swapaxes(-1, -2)], axis=1)
    return dict(zip(ATT_NAMES, (dS, da0, dc0, da1, dc1, np.concatenate([dk0, dk1]), d_row_val, d_col_val)))


def _gelu_parts(x):
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(x) * (1.0 / math.sqrt(2.0))).numpy())
    pdf = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return x * cdf, cdf + x * pdf


def edge_scores_backward_ref(args, dS):
    """The closed form of lapwarm_dual_edge_scores_backward in fp64 NumPy: dict of EDGE_NAMES -> arrays."""
    edge, W1, b1, W2, b2, G = (t.detach().numpy().astype(np.float64) for t in args)
    f = edge.reshape(-1, edge.shape[-1])
    O = G.shape[0]
    d = np.moveaxis(dS.detach().numpy().astype(np.float64).reshape(edge.shape[0], O, -1), 1, 2).reshape(-1, O)
    x1 = f @ W1.T + b1
    h1, g1 = _gelu_parts(x1)
    x2 = h1 @ W2.T + b2
    h2, g2 = _gelu_parts(x2)
    dx2 = (d @ G) * g2
    dx1 = (dx2 @ W2) * g1
    return dict(zip(EDGE_NAMES, (dx1.T @ f, dx1.sum(0), dx2.T @ h1, dx2.sum(0), d.T @ h2)))


def max_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) if np.size(want) else 0.0
