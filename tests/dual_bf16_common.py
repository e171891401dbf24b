"""The arithmetic contract of the bf16 edge MLP (gnn/dual_gnn.py, fused_edge_precision = "bf16") restated in torch --
TEST INFRASTRUCTURE, no project kernel in it.

Round-to-nearest-even conversions to bf16 of: edge_feat, W1, W2, G, h1 = keep scale gelu(x1), h2 = gelu(x2).  Everything
else (b1, b2, x1, x2, GELU, the score) in the dtype of the restatement:

    edge_scores(..., dtype=torch.float64)             the reference of the forward
    edge_scores(..., dtype=torch.float64, ste=True)   the same values, rounding straight-through for autograd
                                                      (x + (round(x) - x).detach()): the reference of the backward
    edge_scores(..., dtype=torch.float32, permute=g)  the stand-in: fp32 sums in a permuted order, the yardstick that
                                                      shows what a correct fp32-accumulating kernel can reach
"""
import torch

EDGE_HIDDEN = 128
ONEGNN_ABS = 1e-5      # the loosest absolute bound the project grants a score
SHARE_CAP = 0.01       # criterion (b): the share of scores further than ONEGNN_ABS from the fp64 restatement
SEED = 20261


def round_bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def _round(x, ste):
    return x + (round_bf16(x) - x).detach() if ste else round_bf16(x)


def _linear(x, W, b, perm):
    if perm is not None:  # the same sum in another order
        idx = perm[perm < x.shape[-1]]
        x, W = x[..., idx], W[:, idx]
    y = x @ W.T
    return y if b is None else y + b


def edge_scores(edge, W1, b1, W2, b2, G, mask0=None, *, dtype=torch.float64, ste=False, permute=None, parts=False):
    """scores (B, 2 H, N, N) from edge (B, N, N, 10); mask0 (B, N, N, 128): scale or 0 per element of h1, or None.
    permute: a torch.Generator; every product then sums over a random permutation of its k index.
    parts: also return max|h2| and max|round(G)| for the flip bound."""
    edge, W1, b1, W2, b2, G = (t.to(dtype) for t in (edge, W1, b1, W2, b2, G))
    perm = None if permute is None else torch.randperm(EDGE_HIDDEN, generator=permute)
    gelu = torch.nn.functional.gelu
    h1 = gelu(_linear(_round(edge, False), _round(W1, ste), b1, perm))
    if mask0 is not None:
        h1 = h1 * mask0.to(dtype)
    h1 = _round(h1, ste)
    h2 = _round(gelu(_linear(h1, _round(W2, ste), b2, perm)), ste)
    Gr = _round(G, ste)
    s = _linear(h2, Gr, None, perm).permute(0, 3, 1, 2).contiguous()
    if parts:
        return s, float(h2.detach().abs().max()), float(Gr.detach().abs().max())
    return s


def flip_bound(h2_max, g_max):
    """B = 2^-7 max|G| max|h2|: two worst-case flips of a rounded h2, each moving a score by up to 2^-8 |h2| |g|."""
    return 2.0 ** -7 * g_max * h2_max


def edge_gradients(edge, W1, b1, W2, b2, G, dS, mask0=None):
    """fp64 autograd through the straight-through restatement: dict W1, b1, W2, b2, G -> gradients.  dS (B, 2 H, N, N);
    an entry of dS that is 0 (outside a prefix) takes its edge out of every sum."""
    leaves = [t.detach().double().requires_grad_(True) for t in (W1, b1, W2, b2, G)]
    s = edge_scores(edge, *leaves, mask0, dtype=torch.float64, ste=True)
    s.backward(dS.double())
    return {name: t.grad for name, t in zip(("W1", "b1", "W2", "b2", "G"), leaves)}


def inputs(B, N, heads, seed=SEED, hidden=None):
    """A default-initialised DualLayer (nn.Linear initialisation), edge features N(0, 1) with channel 0 uniform on
    [0, 3), G folded from projections of random embeddings: (edge, W1, b1, W2, b2, G), float32 on the CPU."""
    from gnn.dual_gnn import DualLayer
    hidden = hidden or 16 * heads
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * N + heads)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed + heads)
    layer = DualLayer(hidden, heads=heads)
    torch.random.set_rng_state(state)
    edge = torch.randn((B, N, N, 10), generator=g)
    edge[..., 0] = 3.0 * torch.rand((B, N, N), generator=g)
    emb = torch.randn((2, B, N, hidden), generator=g)
    with torch.no_grad():
        fold = layer.folded_parameters(layer.row_proj(emb[0]), layer.col_proj(emb[1]))
    lin1, lin2 = layer.edge_mlp[0], layer.edge_mlp[3]
    return tuple(t.detach().clone().contiguous() for t in
                 (edge, lin1.weight, lin1.bias, lin2.weight, lin2.bias, fold["G"]))


def prefix_mask(sizes, N):
    """(B, N, N) bool: i, j < sizes[b] (a size outside 1..N: empty)."""
    n = torch.tensor([s if 1 <= s <= N else 0 for s in sizes])
    inside = torch.arange(N)[None, :] < n[:, None]
    return inside[:, :, None] & inside[:, None, :]


def share_and_max(got, want, inside=None):
    """(share of entries with |got - want| > ONEGNN_ABS, max |got - want|) over `inside` (all entries when None)."""
    diff = (got.double() - want.double()).abs()
    if inside is not None:
        diff = diff[inside]
    return float((diff > ONEGNN_ABS).double().mean()), float(diff.max())


RAGGED_SIZES, RAGGED_N = [1, 16, 17, 33, 0], 33
# (B, N, heads) of the forward: fewer edges than a wave tile; two workgroup tiles and a tail; N = 33 with the three
# paddings of G; more edges than one pass of 256 workgroups x 128 edges
FORWARD_SHAPES = [(1, 5, 4), (2, 12, 4), (1, 33, 1), (1, 33, 4), (1, 33, 8), (2, 130, 4)]
# (B, N, heads) of the backward: 30 976 edges at N = 176, one wave tile past the 30 720-edge chunk
BACKWARD_SHAPES = [(1, 5, 4), (2, 12, 1), (2, 12, 8), (1, 176, 4)]
GRAD_CAP = 2.0 ** -6   # four stacked bf16 half-ulps: no bound of a gradient may exceed it
