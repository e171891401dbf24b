"""DualGNN: graph attention over the O(n^2) edge features in both directions, predicting u and a v hint.

Same constructor arguments, parameter names and shapes (reference state dicts load unchanged), call signature
and output dict {"u", "v_hint"} as the reference module (gnn/dual_gnn.py:17-204).

Two forwards:

  * the FUSED path, taken when the module is in eval mode, the tensors are on CUDA, heads <= 8 and no gradient
    is being recorded.  The reference materialises per layer a (B, N, N, hidden) edge embedding, two
    (B, H, N, N, 3 head_dim) attention inputs and two attention matrices.  The edge embedding enters the layer
    only through the attention scores, which are linear in it, so the last Linear(128, hidden) of the edge MLP
    folds into the score weights (DualLayer.folded_parameters, DESIGN.md "DualGNN"):

        score_row[h,i,j] = leaky_relu(a_h(i) + c_h(j) + g_h . h2(i,j) + k_h)

    with h2 the 128-wide output of the edge MLP's second GELU.  Two HIP kernels do the rest (dual_gnn.hip):
    lapwarm_dual_edge_scores (10 -> 128 -> 128 -> 2 heads per edge on the fp32 MFMA units) and
    lapwarm_dual_attention (masked softmax and the weighted sum of the values, both directions).  The four
    projections, the update MLPs and the LayerNorms stay with PyTorch-ROCm.  The path runs in float32 with
    autocast DISABLED around it: a caller's `torch.autocast("cuda")` is ignored.  Reduced precision is chosen by a
    switch of its own, `fused_edge_precision` (below), never by the autocast context.

  * the plain torch path otherwise (training mode, CPU tensors, a gradient being recorded, heads > 8), in the
    reference's op order with its dropout placements: inside the edge MLP, on both attention-weight tensors and
    in the two update MLPs.

  * with `fused_attention_training = True` (on a DualGNN: all its layers; on a DualLayer used alone: that layer)
    the fused path is also taken in training mode and while a gradient is recorded, as long as `edge_feat` itself
    needs no gradient.  Two autograd functions carry it: _EdgeScores (lapwarm_dual_edge_scores_backward: the edge
    MLP is recomputed per chunk of edges on the MFMA units, gradients for its first two Linears and the folded G)
    and _EdgeAttention (lapwarm_dual_attention_backward from the saved scores, messages and per-query softmax
    statistics: dS, da, dc, dkb, dval).  folded_parameters is differentiable torch, so autograd carries dG, da, dc
    and dkb on to attn_*_weight, attn_*_bias, edge_mlp[5], row_proj and col_proj.  No (B, N, N, hidden) tensor is
    saved: per layer the scores, two messages and 4 B H N statistics.  DROPOUT on this path: the dropouts of the
    two update MLPs are applied as always; the two inside the fused region (in the edge MLP, on the attention
    weights) are applied only with `fused_dropout` (below).  The default, False, routes exactly as before.

  * with `fused_dropout = True` as well (DualGNN: all layers; DualLayer: that layer; default False, and off it changes
    neither routing nor bits) the fused training path applies those two dropouts in training mode when their p is in
    (0, 1): the reference's training regime.  The kernels hold a counter-based generator (csrc/dual_dropout.hpp:
    Philox4x32-10 keyed by a 64-bit seed; an element is kept iff its word >= floor(p 2^32) and then scaled by
    float(1 / (1 - p)); the element index is that of the PADDED (B, N, N, 128) tensor of the edge MLP, stream 0, or of
    the (B, 2, H, N, N) attention weights, stream 1, so tiling, chunking and `sizes` cannot change a mask).  Each
    such layer call draws ONE seed, torch.randint(0, 2**63 - 1, (1,), dtype=torch.int64, generator=g) on the CPU
    with g = `dropout_generator` (None: torch's default CPU generator), the layers in forward order, without any
    device synchronisation.  The seed and p ride on the autograd contexts and the backward REGENERATES the mask:
    no (B, N, N, 128) mask is stored.  A captured graph (torch.cuda.graph) holds the seeds as kernel arguments:
    every replay applies the one mask of the capture.  p == 1 takes the plain path; eval mode never applies them.

  * `fused_edge_precision = "bf16"` (DualGNN: all layers; DualLayer: that layer; default "fp32", which changes neither
    routing nor kernels nor bits) runs the edge MLP, and only it, on the bf16 MFMA units wherever the fused path is
    taken: the eval forward, uniform and with `sizes`, and _EdgeScores with and without `fused_dropout`
    (lapwarm_dual_edge_scores_bf16 and its backward).  Round-to-nearest-even conversions from fp32 to bf16 are applied
    to edge_feat as it is loaded, to W1, W2 and G as they are staged, to h1 after GELU and dropout, to h2 after GELU,
    and in the backward to dS, dh2pre, dh1pre and the column of ones where they become MFMA operands; biases,
    pre-activations, GELU, GELU', the scores and every gradient sum stay fp32 (fp64 across workgroups and chunks).
    The backward recomputes the forward's rounded activations and returns the gradient of the fp32 function at them
    (straight-through rounding); the switch rides on the autograd context.  The attention kernels, the folded a, c
    and kbias and everything torch does stay fp32; the dropout mask of a seed is the mask under "fp32".  The seeds
    feed an exact fp64 solver: a less precise u changes the number of augmenting paths, never the optimal cost.

A padded batch of instances of different sizes passes `sizes` (B,) int32 on the device: `mask` is then the prefix
mask of the sizes (built here when it is None).  The fused path hands the sizes to lapwarm_dual_edge_scores_ragged
and lapwarm_dual_attention_ragged, which skip the padding: the edge MLP runs on the edges (i, j < n_b) only, and
the attention neither loads a score nor walks a key tile outside a prefix.  The outputs are, bit for bit, those of
the same call without `sizes`.  On the plain path `sizes` only supplies the mask.

The backward kernels are deterministic (fixed-order sums, no atomics): equal inputs give equal gradients.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .features import EDGE_FEATURE_DIM, NODE_FEATURE_DIM

FUSED_MAX_HEADS = 8
EDGE_HIDDEN = 128


def _records_grad(module, *tensors) -> bool:
    if not torch.is_grad_enabled():
        return False
    return any(t.requires_grad for t in tensors) or any(p.requires_grad for p in module.parameters())


def _prefix_mask(sizes, mask, edge_feat) -> torch.Tensor:
    """The (B, N) prefix mask of `sizes` after checking them, and `mask` against it when one is given."""
    B, N = edge_feat.shape[:2]
    if not isinstance(sizes, torch.Tensor) or sizes.dtype != torch.int32:
        raise TypeError("sizes must be a torch.int32 tensor")
    if tuple(sizes.shape) != (B,) or not sizes.is_contiguous():
        raise ValueError(f"sizes must be a contiguous ({B},) tensor, not {tuple(sizes.shape)}")
    if sizes.device != edge_feat.device:
        raise ValueError(f"sizes must be on {edge_feat.device} like the features, not {sizes.device}")
    inside = (sizes >= 1) & (sizes <= N)
    prefix = torch.arange(N, device=sizes.device).unsqueeze(0) < torch.where(inside, sizes, 0).unsqueeze(1)
    if mask is not None and (tuple(mask.shape) != (B, N) or not torch.equal(mask.to(prefix.device, torch.bool), prefix)):
        raise ValueError("mask is not the prefix mask of sizes")
    return prefix


def _edge_precision(value) -> str:
    if value not in ("fp32", "bf16"):
        raise ValueError(f'fused_edge_precision must be "fp32" or "bf16", not {value!r}')
    return value


def _backward_workspace(lib, B, N, H, dev) -> torch.Tensor:
    nbytes = int(lib.lapwarm_dual_backward_workspace_bytes(B, N, H))
    if nbytes == 0:
        raise ValueError(f"DualLayer: batch {B}, n {N} or heads {H} outside the fused kernels' range")
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


# ---- which C entry a fused call reaches: each choice is made here and nowhere else ------------------------------
def _edge_scores_entry(sizes, seed, p, precision, dims):
    """The entry that computes the edge scores of (sizes, p, precision) and its arguments after `scores`; dims is
    (B, N, H).  fp32 without dropout keeps the plain and the _ragged entry: timings and profiles name them."""
    if precision == "bf16":  # one entry for both batches: sizes may be None, p == 0 is no dropout
        return "lapwarm_dual_edge_scores_bf16", (sizes, *dims, seed, p)
    if p > 0.0:  # the dropout after the edge MLP's first GELU, stream 0 of the seed
        return "lapwarm_dual_edge_scores_dropout", (sizes, *dims, seed, p)
    if sizes is not None:
        return "lapwarm_dual_edge_scores_ragged", (sizes, *dims)
    return "lapwarm_dual_edge_scores", tuple(dims)


def _edge_backward_entry(seed, p, precision):
    """The backward of _edge_scores_entry's entry and its arguments after the workspace: the forward's precision, and
    its mask again from its seed."""
    suffix = "_bf16" if precision == "bf16" else "_dropout" if p > 0.0 else ""
    return "lapwarm_dual_edge_scores_backward" + suffix, ((seed, p) if suffix else ())


def _attention_entry(mask8, sizes, seed, p, stats):
    """The attention forward of (sizes, p): the entry, its arguments between kbias and the values, and those after
    (B, N, H, D).  stats: the training forward, which keeps the softmax statistics; only it has a dropout."""
    if p > 0.0:  # the dropout of the attention weights, stream 1 of the seed
        assert stats
        return "lapwarm_dual_attention_stats_dropout", (mask8, sizes), (seed, p)
    name = "lapwarm_dual_attention_stats" if stats else "lapwarm_dual_attention"
    if sizes is not None:  # scores outside the prefixes are neither written nor read
        return name + "_ragged", (sizes,), ()
    return name, (mask8,), ()


def _attention_backward_entry(seed, p):
    """The backward of _attention_entry's entry (it takes mask8 and sizes always) and its arguments after the workspace."""
    return ("lapwarm_dual_attention_backward_dropout", (seed, p)) if p > 0.0 else ("lapwarm_dual_attention_backward", ())


class _EdgeScores(torch.autograd.Function):
    """scores (B, 2, H, N, N) of lapwarm_dual_edge_scores[_ragged]; saves only its inputs.  The backward is
    lapwarm_dual_edge_scores_backward: gradients for W1, b1, W2, b2 and G, none for edge_feat.  With `sizes` the
    scores outside the prefixes are never written and their gradient is never read."""

    @staticmethod
    def forward(ctx, edge_feat, W1, b1, W2, b2, G, sizes, seed=0, p=0.0, precision="fp32"):
        from lap import _hip
        from ._call import hip_call
        _hip.require_device()
        B, N = edge_feat.shape[:2]
        H = G.shape[0] // 2
        args = [t.detach().contiguous() for t in (edge_feat, W1, b1, W2, b2, G)]
        scores = torch.empty((B, 2, H, N, N), dtype=torch.float32, device=edge_feat.device)
        entry, tail = _edge_scores_entry(sizes, seed, p, precision, (B, N, H))
        hip_call(entry, "dual_edge_scores", scores.device, *args, scores, *tail)
        ctx.save_for_backward(*args)
        ctx.sizes, ctx.seed, ctx.p, ctx.precision = sizes, seed, p, precision
        return scores

    @staticmethod
    def backward(ctx, d_scores):
        from lap import _hip
        from ._call import hip_call
        edge_feat, W1, b1, W2, b2, G = ctx.saved_tensors
        B, N = edge_feat.shape[:2]
        H = G.shape[0] // 2
        dev = edge_feat.device
        ws = _backward_workspace(_hip.load(), B, N, H, dev)
        grads = [torch.empty_like(t) for t in (W1, b1, W2, b2, G)]
        entry, tail = _edge_backward_entry(ctx.seed, ctx.p, ctx.precision)
        hip_call(entry, "dual_edge_scores_backward", dev, edge_feat, W1, b1, W2, b2, G, d_scores.contiguous(), ctx.sizes,
                 *grads, B, N, H, ws, ws.numel(), *tail)
        return (None, *grads, None, None, None, None)


class _EdgeAttention(torch.autograd.Function):
    """(row_msg, col_msg) of lapwarm_dual_attention_stats[_ragged]; saves the scores, the per-query softmax
    statistics and the messages.  The backward is lapwarm_dual_attention_backward."""

    @staticmethod
    def forward(ctx, scores, a_row, c_row, a_col, c_col, kbias, row_val, col_val, mask8, sizes, seed=0, p=0.0):
        from lap import _hip
        from ._call import hip_call
        _hip.require_device()
        B, _, H, N, _ = scores.shape
        D = row_val.shape[-1] // H
        dev = scores.device
        args = [t.detach().contiguous() for t in (scores, a_row, c_row, a_col, c_col, kbias)]
        vals = [t.detach().contiguous() for t in (row_val, col_val)]
        row_msg, col_msg = (torch.empty((B, N, H * D), dtype=torch.float32, device=dev) for _ in range(2))
        row_stats, col_stats = (torch.empty((B, H, N, 2), dtype=torch.float32, device=dev) for _ in range(2))
        entry, masks, tail = _attention_entry(mask8, sizes, seed, p, stats=True)
        hip_call(entry, "dual_attention", dev, *args, *masks, *vals, row_msg, col_msg, row_stats, col_stats, B, N, H, D,
                 *tail)
        ctx.save_for_backward(*args, *vals, row_msg, col_msg, row_stats, col_stats)
        ctx.mask8, ctx.sizes, ctx.seed, ctx.p = mask8, sizes, seed, p
        return row_msg, col_msg

    @staticmethod
    def backward(ctx, d_row_msg, d_col_msg):
        from lap import _hip
        from ._call import hip_call
        (scores, a_row, c_row, a_col, c_col, kbias, row_val, col_val, row_msg, col_msg, row_stats,
         col_stats) = ctx.saved_tensors
        B, _, H, N, _ = scores.shape
        D = row_val.shape[-1] // H
        dev = scores.device
        ws = _backward_workspace(_hip.load(), B, N, H, dev)
        # with sizes the kernel leaves dS outside the prefixes alone: zeros there, so the tensor is a clean gradient
        dS = (torch.zeros_like if ctx.sizes is not None else torch.empty_like)(scores)
        da_row, dc_row, da_col, dc_col = (torch.empty_like(a_row) for _ in range(4))
        dkb = torch.empty_like(kbias)
        d_row_val, d_col_val = torch.empty_like(row_val), torch.empty_like(col_val)
        entry, tail = _attention_backward_entry(ctx.seed, ctx.p)
        hip_call(entry, "dual_attention_backward", dev, scores, a_row, c_row, a_col, c_col, kbias, ctx.mask8, ctx.sizes, row_val, col_val, row_msg, col_msg,
                 row_stats, col_stats, d_row_msg.contiguous(), d_col_msg.contiguous(), dS, da_row, dc_row, da_col,
                 dc_col, dkb, d_row_val, d_col_val, B, N, H, D, ws, ws.numel(), *tail)
        return dS, da_row, dc_row, da_col, dc_col, dkb, d_row_val, d_col_val, None, None, None, None


class DualLayer(nn.Module):
    # With True, CUDA float32 tensors with heads <= 8 and an edge_feat that needs no gradient take the fused path
    # also in training mode and while a gradient is recorded (HIP forward and backward).  The two dropouts inside
    # the fused region (in the edge MLP, on the attention weights) are then not applied unless fused_dropout is set
    # too; those of the update MLPs are.  DualGNN.fused_attention_training sets it on every layer of a model.
    fused_attention_training = False
    # With True as well, the fused training path applies the two dropouts of the fused region in training mode
    # (module docstring): one seed per layer call from `dropout_generator` (a CPU torch.Generator, or None for torch's
    # default one), the masks regenerated in the backward.  DualGNN.fused_dropout / .dropout_generator set both on
    # every layer of a model.
    fused_dropout = False
    dropout_generator = None
    # "fp32" or "bf16": the arithmetic of the edge MLP wherever the fused path is taken (module docstring).  Checked
    # when a fused call reads it; DualGNN.fused_edge_precision checks it when it is set.
    fused_edge_precision = "fp32"

    def __init__(self, hidden_dim: int, heads: int = 4, dropout: float = 0.1) -> None:
        super().__init__()
        if hidden_dim % heads != 0:
            raise ValueError("hidden_dim must be divisible by number of heads")
        self.heads = heads
        self.head_dim = hidden_dim // heads
        self.edge_mlp = nn.Sequential(
            nn.Linear(EDGE_FEATURE_DIM, EDGE_HIDDEN), nn.GELU(), nn.Dropout(dropout),
            nn.Linear(EDGE_HIDDEN, EDGE_HIDDEN), nn.GELU(),
            nn.Linear(EDGE_HIDDEN, hidden_dim))
        self.row_proj = nn.Linear(hidden_dim, hidden_dim, bias=False)
        self.col_proj = nn.Linear(hidden_dim, hidden_dim, bias=False)
        self.row_val = nn.Linear(hidden_dim, hidden_dim, bias=False)
        self.col_val = nn.Linear(hidden_dim, hidden_dim, bias=False)
        self.attn_row_weight = nn.Parameter(torch.empty(heads, self.head_dim * 3))
        self.attn_col_weight = nn.Parameter(torch.empty(heads, self.head_dim * 3))
        self.attn_row_bias = nn.Parameter(torch.zeros(heads))
        self.attn_col_bias = nn.Parameter(torch.zeros(heads))
        self.dropout = nn.Dropout(dropout)
        self.leaky_relu = nn.LeakyReLU(0.2)
        self.row_update = nn.Sequential(nn.Linear(hidden_dim * 2, hidden_dim), nn.GELU(), nn.Dropout(dropout))
        self.col_update = nn.Sequential(nn.Linear(hidden_dim * 2, hidden_dim), nn.GELU(), nn.Dropout(dropout))
        self.row_norm = nn.LayerNorm(hidden_dim)
        self.col_norm = nn.LayerNorm(hidden_dim)
        nn.init.xavier_uniform_(self.attn_row_weight)
        nn.init.xavier_uniform_(self.attn_col_weight)

    # ---- the folding ---------------------------------------------------------------------------------------
    def folded_parameters(self, row_proj: torch.Tensor, col_proj: torch.Tensor) -> dict:
        """What the fused path passes to the kernels, from the projections (B, N, hidden) and the parameters:
        a_row, c_row, a_col, c_col (B, H, N), G (2 H, 128) and kbias (2 H,), rows 0..H-1 the row direction.
        attn_row_weight[h] = [w_r | w_c | w_e]; attn_col_weight[h] = [w_c | w_r | w_e]."""
        H, D = self.heads, self.head_dim
        B, N, _ = row_proj.shape
        rp, cp = row_proj.reshape(B, N, H, D), col_proj.reshape(B, N, H, D)
        W3 = self.edge_mlp[5].weight.reshape(H, D, EDGE_HIDDEN)
        b3 = self.edge_mlp[5].bias.reshape(H, D)
        wr, wc = self.attn_row_weight, self.attn_col_weight
        g_row = torch.einsum("hd,hdk->hk", wr[:, 2 * D:], W3)
        g_col = torch.einsum("hd,hdk->hk", wc[:, 2 * D:], W3)
        k_row = (wr[:, 2 * D:] * b3).sum(-1) + self.attn_row_bias
        k_col = (wc[:, 2 * D:] * b3).sum(-1) + self.attn_col_bias
        return {
            "a_row": torch.einsum("bnhd,hd->bhn", rp, wr[:, :D]).contiguous(),
            "c_row": torch.einsum("bnhd,hd->bhn", cp, wr[:, D:2 * D]).contiguous(),
            "a_col": torch.einsum("bnhd,hd->bhn", cp, wc[:, :D]).contiguous(),
            "c_col": torch.einsum("bnhd,hd->bhn", rp, wc[:, D:2 * D]).contiguous(),
            "G": torch.cat([g_row, g_col], 0).contiguous(),
            "kbias": torch.cat([k_row, k_col], 0).contiguous(),
        }

    def _messages_fused(self, edge_feat, row_embed, col_embed, mask, sizes=None):
        from lap import _hip
        from ._call import hip_call
        lib = _hip.require_device()
        B, N = edge_feat.shape[:2]
        H, D = self.heads, self.head_dim
        dev = edge_feat.device
        fold = self.folded_parameters(self.row_proj(row_embed), self.col_proj(col_embed))
        row_val = self.row_val(row_embed).contiguous()
        col_val = self.col_val(col_embed).contiguous()
        nbytes = int(lib.lapwarm_dual_gnn_workspace_bytes(B, N, H))
        if nbytes == 0:
            raise ValueError(f"DualLayer: batch {B}, n {N} or heads {H} outside the fused kernels' range")
        lin1, lin2 = self.edge_mlp[0], self.edge_mlp[3]
        precision = _edge_precision(self.fused_edge_precision)
        p_edge, p_attn = self._fused_dropout_rates()
        dropout = p_edge > 0.0 or p_attn > 0.0
        edge = (edge_feat, lin1.weight, lin1.bias, lin2.weight, lin2.bias, fold["G"])
        attn = (fold["a_row"], fold["c_row"], fold["a_col"], fold["c_col"], fold["kbias"])
        mask8 = None if mask is None or sizes is not None else mask.to(torch.uint8).contiguous()
        if dropout or _records_grad(self, row_embed, col_embed):  # the trainable route: HIP forward and backward
            seed = 0
            if dropout:  # one seed per layer call, on the CPU: no device synchronisation
                seed = int(torch.randint(0, 2**63 - 1, (1,), dtype=torch.int64, generator=self.dropout_generator))
            scores = _EdgeScores.apply(*edge, sizes, seed, p_edge, precision)
            return _EdgeAttention.apply(scores, *attn, row_val, col_val, mask8, sizes, seed, p_attn)
        row_msg = torch.empty((B, N, H * D), dtype=torch.float32, device=dev)
        col_msg = torch.empty((B, N, H * D), dtype=torch.float32, device=dev)
        scores = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        entry, tail = _edge_scores_entry(sizes, 0, 0.0, precision, (B, N, H))  # seed 0, p 0: no dropout
        hip_call(entry, "dual_edge_scores", dev, *edge, scores, *tail)
        entry, masks, tail = _attention_entry(mask8, sizes, 0, 0.0, stats=False)
        hip_call(entry, "dual_attention", dev, scores, *attn, *masks, row_val, col_val, row_msg, col_msg, B, N, H, D, *tail)
        return row_msg, col_msg

    # ---- the plain path ------------------------------------------------------------------------------------
    def _attend(self, first, second, edge, weight, bias, keep, values, transpose):
        """One direction: scores from [first | second | edge] . weight + bias over (B, H, query, key)."""
        x = torch.cat([first, second, edge], dim=-1)
        x = x.permute(0, 3, 2, 1, 4) if transpose else x.permute(0, 3, 1, 2, 4)
        s = torch.einsum("bhijm,hm->bhij", x, weight) + bias[None, :, None, None]
        s = self.leaky_relu(s)
        s = s.masked_fill(~keep[:, None, :, None], float("-inf"))
        s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
        w = torch.softmax(s, dim=-1)
        w = torch.where(torch.isfinite(w), w, torch.zeros_like(w))  # a fully masked query: zero message
        w = self.dropout(w)
        out = torch.einsum("bhij,bhjd->bhid", w, values.permute(0, 2, 1, 3))
        B, _, N, _ = out.shape
        return out.permute(0, 2, 1, 3).reshape(B, N, -1)

    def _messages_plain(self, edge_feat, row_embed, col_embed, mask):
        B, N = edge_feat.shape[:2]
        H, D = self.heads, self.head_dim
        keep = mask if mask is not None else edge_feat.new_ones((B, N), dtype=torch.bool)
        rp = self.row_proj(row_embed).view(B, N, H, D)
        cp = self.col_proj(col_embed).view(B, N, H, D)
        rv = self.row_val(row_embed).view(B, N, H, D)
        cv = self.col_val(col_embed).view(B, N, H, D)
        edge = self.edge_mlp(edge_feat).view(B, N, N, H, D)
        rows = rp.unsqueeze(2).expand(B, N, N, H, D)
        cols = cp.unsqueeze(1).expand(B, N, N, H, D)
        row_msg = self._attend(rows, cols, edge, self.attn_row_weight, self.attn_row_bias, keep, cv, False)
        col_msg = self._attend(cols, rows, edge, self.attn_col_weight, self.attn_col_bias, keep, rv, True)
        return row_msg, col_msg

    def _fused_dropout_rates(self) -> tuple[float, float]:
        """(p of the edge MLP's dropout, p of the attention weights' dropout) as the fused path applies them: 0 where
        fused_dropout is off, in eval mode, or for a p outside (0, 1)."""
        if not (self.fused_dropout and self.fused_attention_training and self.training):
            return 0.0, 0.0
        return tuple(float(m.p) if 0.0 < m.p < 1.0 else 0.0 for m in (self.edge_mlp[2], self.dropout))

    def takes_fused_path(self, edge_feat, row_embed, col_embed) -> bool:
        fits = (edge_feat.is_cuda and self.heads <= FUSED_MAX_HEADS
                and self.attn_row_weight.dtype == torch.float32)  # (a .double() copy is a plain-path model)
        if self.fused_dropout and self.training and max(self.edge_mlp[2].p, self.dropout.p) >= 1.0:
            return False  # p == 1 drops everything: the plain path
        if self.fused_attention_training:  # training mode and recorded gradients too; none for edge_feat
            return fits and not (torch.is_grad_enabled() and edge_feat.requires_grad)
        return fits and not self.training and not _records_grad(self, edge_feat, row_embed, col_embed)

    def forward(self, edge_feat: torch.Tensor, row_embed: torch.Tensor, col_embed: torch.Tensor,
                mask: Optional[torch.Tensor], sizes: Optional[torch.Tensor] = None
                ) -> tuple[torch.Tensor, torch.Tensor]:
        """`sizes` (B,) int32 on the device of the tensors: `mask` is their prefix mask (DualGNN.forward checks it)."""
        if self.takes_fused_path(edge_feat, row_embed, col_embed):
            with torch.autocast("cuda", enabled=False):
                edge_feat = edge_feat.float().contiguous()
                row_embed, col_embed = row_embed.float(), col_embed.float()
                row_msg, col_msg = self._messages_fused(edge_feat, row_embed, col_embed, mask, sizes)
                return self._update(row_embed, col_embed, row_msg, col_msg)
        row_msg, col_msg = self._messages_plain(edge_feat, row_embed, col_embed, mask)
        return self._update(row_embed, col_embed, row_msg, col_msg)

    def _update(self, row_embed, col_embed, row_msg, col_msg):
        row_new = self.row_update(torch.cat([row_embed, row_msg], dim=-1))
        col_new = self.col_update(torch.cat([col_embed, col_msg], dim=-1))
        return self.row_norm(row_embed + row_new), self.col_norm(col_embed + col_new)


class DualGNN(nn.Module):
    def __init__(self, hidden_dim: int = 128, layers: int = 4, heads: int = 4, dropout: float = 0.1) -> None:
        super().__init__()
        if layers <= 0:
            raise ValueError("DualGNN must have at least one layer")
        self.hidden_dim = hidden_dim
        self.heads = heads
        self.row_encoder = nn.Sequential(nn.Linear(NODE_FEATURE_DIM, hidden_dim), nn.GELU(), nn.LayerNorm(hidden_dim))
        self.col_encoder = nn.Sequential(nn.Linear(NODE_FEATURE_DIM, hidden_dim), nn.GELU(), nn.LayerNorm(hidden_dim))
        self.layers = nn.ModuleList([DualLayer(hidden_dim, heads=heads, dropout=dropout) for _ in range(layers)])
        self.row_out = nn.Linear(hidden_dim, 1)
        self.col_out = nn.Linear(hidden_dim, 1)

    @property
    def fused_attention_training(self) -> bool:
        """The switch of every layer (DualLayer.fused_attention_training); False unless set."""
        return all(layer.fused_attention_training for layer in self.layers)

    @fused_attention_training.setter
    def fused_attention_training(self, on: bool) -> None:
        for layer in self.layers:
            layer.fused_attention_training = bool(on)

    @property
    def fused_dropout(self) -> bool:
        """The switch of every layer (DualLayer.fused_dropout); False unless set."""
        return all(layer.fused_dropout for layer in self.layers)

    @fused_dropout.setter
    def fused_dropout(self, on: bool) -> None:
        for layer in self.layers:
            layer.fused_dropout = bool(on)

    @property
    def fused_edge_precision(self) -> str:
        """The switch of every layer (DualLayer.fused_edge_precision): "fp32" unless set; "bf16" when all layers are."""
        return "bf16" if all(layer.fused_edge_precision == "bf16" for layer in self.layers) else "fp32"

    @fused_edge_precision.setter
    def fused_edge_precision(self, precision: str) -> None:
        precision = _edge_precision(precision)
        for layer in self.layers:
            layer.fused_edge_precision = precision

    @property
    def dropout_generator(self) -> Optional[torch.Generator]:
        """The CPU generator the layers draw their dropout seeds from, in forward order; None: torch's default."""
        return self.layers[0].dropout_generator

    @dropout_generator.setter
    def dropout_generator(self, generator: Optional[torch.Generator]) -> None:
        for layer in self.layers:
            layer.dropout_generator = generator

    def _forward(self, edge_feat, row_feat, col_feat, mask, sizes=None):
        nodes = (self.row_encoder(row_feat), self.col_encoder(col_feat))
        for layer in self.layers:
            nodes = layer(edge_feat, *nodes, mask, sizes)
        u, v_hint = (head(x).squeeze(-1) for head, x in zip((self.row_out, self.col_out), nodes))
        # the gauge: u is centred per instance (over all N slots, padded ones included, as the reference does) and
        # v_hint takes the mean, so that u_i + v_j is unchanged
        shift = u.mean(dim=-1, keepdim=True)
        u, v_hint = u - shift, v_hint + shift
        if mask is not None:
            u, v_hint = (t.masked_fill(~mask, 0.0) for t in (u, v_hint))
        return {"u": u, "v_hint": v_hint}

    def forward(self, edge_feat: torch.Tensor, row_feat: torch.Tensor, col_feat: torch.Tensor,
                mask: Optional[torch.Tensor] = None, *, sizes: Optional[torch.Tensor] = None
                ) -> dict[str, torch.Tensor]:
        """`sizes`: (B,) int32 on the device of the features, the size of every instance of a padded batch (a size
        outside 1..N is an empty instance).  `mask` must then be None or the prefix mask of the sizes; comparing a
        given mask reads one flag back from the device."""
        if edge_feat.ndim != 4:
            raise ValueError("edge_feat must have shape (batch, n, n, F)")
        if sizes is not None:
            mask = _prefix_mask(sizes, mask, edge_feat)
        if self.layers[0].takes_fused_path(edge_feat, row_feat, col_feat) and (
                self.fused_attention_training or not _records_grad(self)):
            # float32 end to end, whatever autocast context the caller is in
            with torch.autocast("cuda", enabled=False):
                return self._forward(edge_feat.float(), row_feat.float(), col_feat.float(), mask, sizes)
        return self._forward(edge_feat, row_feat, col_feat, mask, sizes)


__all__ = ["DualGNN", "DualLayer", "EDGE_FEATURE_DIM", "NODE_FEATURE_DIM", "FUSED_MAX_HEADS"]
