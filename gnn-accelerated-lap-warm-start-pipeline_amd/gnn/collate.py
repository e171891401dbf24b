"""`collate_device`: the reference's `collate` (gnn/train_one_gnn.py:72-91) and `collate_mixed_size`
(gnn/train_progressive_clean.py:182-224) for the MI355X.  Instances of different sizes become one padded
batch -- float32 costs, targets, row features, top-16 and mask -- in one ragged call on the device, instead of
one feature call per instance on the host followed by a pad and a cast."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .features import row_features_ragged


@dataclass
class DeviceBatch:
    """A padded batch on the device; N = the largest size.  The fields of the reference's Batch, plus the
    top-16 that OneGNN takes as `topk_values=` and the sizes the mask stands for."""
    cost: torch.Tensor      # (B, N, N) float32, 0 outside the prefix
    u: torch.Tensor         # (B, N) float32, 0 on padded rows
    v: torch.Tensor         # (B, N) float32
    row_feat: torch.Tensor  # (B, N, 21) float32, 0 on padded rows
    topk: torch.Tensor      # (B, N, 16) float32 ascending, +inf beyond n_b and on padded rows
    mask: torch.Tensor      # (B, N) bool, the prefix mask
    sizes: torch.Tensor     # (B,) int32


@dataclass
class DualDeviceBatch:
    """A padded DualGNN batch on the device; N = the largest size.  The fields of the reference's Batch
    (gnn/train.py:33-41), as its `collate` (:64-95) pads them, plus the sizes the mask stands for.  Made by
    DualWarmStartPipeline.dual_training_batch."""
    cost: torch.Tensor       # (B, N, N) float32, 0 outside the prefix
    u: torch.Tensor          # (B, N) float32, 0 on padded rows
    v: torch.Tensor          # (B, N) float32
    row_feat: torch.Tensor   # (B, N, 14) float32, 0 on padded rows
    col_feat: torch.Tensor   # (B, N, 14) float32, 0 on padded columns
    edge_feat: torch.Tensor  # (B, N, N, 10) float32, 0 outside the prefix
    mask: torch.Tensor       # (B, N) bool, the prefix mask
    sizes: torch.Tensor      # (B,) int32


def _host_vector(x, n, name):
    x = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).reshape(-1)
    if x.shape[0] < n:
        raise ValueError(f"'{name}' holds {x.shape[0]} values for an instance of size {n}")
    return x[:n]


def collate_device(items, device="cuda:0") -> DeviceBatch:
    """items: dicts in either of the reference's forms -- `cost` or `C` (n x n, NumPy or tensor), `u`, `v`
    (at least n values) and `n` or `size` (optional: the matrix says it).  One H2D copy of the packed fp64
    costs, one of the offsets and sizes, one of the padded float32 u and v, and two kernels."""
    items = list(items)
    costs = []
    for it in items:
        c = it["cost"] if "cost" in it else it["C"]
        n = it.get("n", it.get("size"))
        if n is not None and (len(c.shape) != 2 or int(n) != c.shape[0]):
            raise ValueError(f"item of size {int(n)} with a cost matrix of shape {tuple(c.shape)}")
        costs.append(c)
    sizes = [int(c.shape[0]) for c in costs]
    N = max(sizes, default=0)
    uv = np.zeros((2, len(items), N), dtype=np.float32)
    for b, (it, n) in enumerate(zip(items, sizes)):
        uv[0, b, :n] = _host_vector(it["u"], n, "u")
        uv[1, b, :n] = _host_vector(it["v"], n, "v")
    r = row_features_ragged(costs, return_topk=True, want_cost32=True, device=device)  # validates first
    uv_d = torch.from_numpy(uv).to(r.feat.device)
    return DeviceBatch(cost=r.cost32, u=uv_d[0], v=uv_d[1], row_feat=r.feat, topk=r.topk, mask=r.mask,
                       sizes=r.sizes)
