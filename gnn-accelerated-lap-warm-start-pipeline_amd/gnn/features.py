"""Row features for OneGNN, computed by the HIP row-sweep kernel (dense_sweeps.hip).

`compute_row_features(C)` keeps the reference's contract (gnn/features.py:161-243): a float64
(n, n) cost matrix in, a float32 (n, 21) descriptor out, (0, 0) for n == 0: 13 fp64 row
statistics cast to float32 followed by 8 positional encodings.

`compute_row_features_torch(cost)` is the device-resident entry the harness' CUDA branch calls
(scripts/gnn_benchmark.py:233-240).  Unlike the reference's torch variant (gnn/features.py:246-351,
float32 maths, ddof=1, argmin-only column counts) it returns exactly the same statistics as
`compute_row_features`, because the same fp64 kernel produces both.

`graph_features_device(C, u=None)` and `compute_features(C, ...)` are DualGNN's O(n^2) features (the reference's
gnn/features.py:49-153): 10 edge channels and 14 row / column statistics, computed in fp64 by graph_features.hip.
Ranks are stable (the lower index first among equal values), which is one of the rankings the reference's
unstable argsort may return.  `graph_features_ragged` / `graph_features_packed` compute them for instances of
different sizes in one call, padded as the reference's collate pads them.  `gnn.compute_features` (the package-level name) still raises; see `gnn`.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from lap import _hip

POS_FREQS = (1, 2, 4, 8)
ROW_FEATURE_DIM = 13 + 2 * len(POS_FREQS)
TOPK = 16
EDGE_FEATURE_DIM = 10
NODE_FEATURE_DIM = 6 + 2 * len(POS_FREQS)
GRAPH_MAX_N = 4096  # a row, its sort keys and indices in LDS (graph_features.hpp)


def positional_encodings(n: int) -> np.ndarray:
    """(n, 8) float32 table, sin/cos(2 pi i f / max(1, n-1)) for f in (1,2,4,8)
    (gnn/features.py:21-31).  O(n) host work, cached per n by the pipeline."""
    if n <= 0:
        return np.zeros((0, 2 * len(POS_FREQS)), dtype=np.float32)
    pos = np.arange(n, dtype=np.float64)
    scale = max(1, n - 1)
    cols = []
    for f in POS_FREQS:
        ang = 2.0 * np.pi * pos * f / scale
        cols.append(np.sin(ang))
        cols.append(np.cos(ang))
    return np.stack(cols, axis=-1).astype(np.float32)


def compute_row_features(C: np.ndarray, return_topk: bool = False):
    """Host arrays in/out; the work happens on the GPU."""
    C = np.ascontiguousarray(np.asarray(C, dtype=np.float64))
    n = C.shape[0]
    if n == 0:
        out = np.zeros((0, 0), dtype=np.float32)
        return (out, np.zeros((0, TOPK), dtype=np.float32)) if return_topk else out
    if C.ndim != 2 or C.shape[1] != n:
        raise ValueError("compute_row_features on the MI355X path expects a square cost matrix")
    lib = _hip.require_device()
    feat = np.empty((n, ROW_FEATURE_DIM), dtype=np.float32)
    topk = np.empty((n, TOPK), dtype=np.float32)
    rc = lib.lapwarm_row_features(C.ctypes.data_as(_hip.c_dp), n, feat.ctypes.data_as(_hip.c_fp),
                                  topk.ctypes.data_as(_hip.c_fp))
    if _hip.check(rc, "compute_row_features") != 0:
        raise RuntimeError(f"compute_row_features failed (code {rc})")
    return (feat, topk) if return_topk else feat


_POSENC_CACHE = {}


def _posenc_device(n: int, device):
    import torch
    key = (n, str(device))
    if key not in _POSENC_CACHE:
        _POSENC_CACHE[key] = torch.from_numpy(positional_encodings(n)).to(device)
    return _POSENC_CACHE[key]


def row_features_device(C, return_topk: bool = True):
    """C: CUDA float64 tensor (B, n, n) or (n, n) -> feat (B, n, 21) f32 [, topk (B, n, 16) f32].
    Enqueued on the current torch stream; no host synchronisation."""
    import torch
    from ._call import hip_call
    if not C.is_cuda or C.dtype != torch.float64:
        raise TypeError("row_features_device expects a CUDA float64 tensor")
    squeeze = C.ndim == 2
    if squeeze:
        C = C.unsqueeze(0)
    C = C.contiguous()
    B, n, m = C.shape
    if n != m or n < 1:
        raise ValueError("square, non-empty cost matrices expected")
    lib = _hip.require_device()
    feat = torch.empty((B, n, ROW_FEATURE_DIM), dtype=torch.float32, device=C.device)
    topk = torch.empty((B, n, TOPK), dtype=torch.float32, device=C.device)
    ws_bytes = lib.lapwarm_sweep_workspace_bytes(B, n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=C.device)
    pos = _posenc_device(n, C.device)
    hip_call("lapwarm_row_features_batched", "row_features_device", C.device, C, B, n, pos, feat, topk, ws, ws_bytes)
    if squeeze:
        feat, topk = feat[0], topk[0]
    return (feat, topk) if return_topk else feat


MAX_N = 16384       # LDS of the row kernels
MAX_BATCH = 65535   # the batch is one grid dimension

_RAGGED_POSENC_CACHE = {}


def _ragged_posenc(distinct, device):
    """The (n, 8) tables of the sizes in `distinct` (sorted), one after the other, on the device, and the first
    row of each: built on the host from positional_encodings, so bit-identical to the per-n tables; kept per
    set of sizes (the newest 32 sets)."""
    import torch
    key = (distinct, str(device))
    if key not in _RAGGED_POSENC_CACHE:
        if len(_RAGGED_POSENC_CACHE) >= 32:
            _RAGGED_POSENC_CACHE.pop(next(iter(_RAGGED_POSENC_CACHE)))
        first = dict(zip(distinct, np.concatenate(([0], np.cumsum(distinct)[:-1])).tolist()))
        table = np.concatenate([positional_encodings(n) for n in distinct], axis=0)
        _RAGGED_POSENC_CACHE[key] = (torch.from_numpy(table).to(device), first)
    return _RAGGED_POSENC_CACHE[key]


_RAGGED_META_CACHE = {}


def _ragged_meta(host_sizes, ld, offsets, device):
    """offsets (B,) int64, sizes and pos_off (B,) int32 and the positional-encoding tables on the device.  They
    depend on the sizes and the layout alone and nothing writes to them, so they are kept per (sizes, ld, device),
    the newest 32: a batch of a shape seen before uploads nothing and waits for nothing."""
    import torch
    key = (host_sizes, ld, str(device))
    hit = _RAGGED_META_CACHE.get(key)
    if hit is None:
        if len(_RAGGED_META_CACHE) >= 32:
            _RAGGED_META_CACHE.pop(next(iter(_RAGGED_META_CACHE)))
        B = len(host_sizes)
        posenc, first = _ragged_posenc(tuple(sorted(set(host_sizes))), device)
        meta = np.empty(2 * B, dtype=np.int64)  # offsets, then sizes and pos_off as int32: one copy
        meta[:B] = offsets
        m32 = meta[B:].view(np.int32)
        m32[:B] = host_sizes
        m32[B:] = [first[n] for n in host_sizes]
        meta_d = torch.from_numpy(meta).to(device)
        d32 = meta_d[B:].view(torch.int32)
        hit = _RAGGED_META_CACHE[key] = (meta_d[:B], d32[:B], d32[B:], posenc)
    return hit


class RaggedFeatures:
    """What one ragged call returns, padded to N = the largest size: feat (B, N, 21) f32, topk (B, N, 16) f32
    or None, cost32 (B, N, N) f32 or None, mask (B, N) bool, sizes (B,) int32 and ret (B,) int32 (0, or 2
    for a size outside 1..N), all on the device."""
    __slots__ = ("feat", "topk", "cost32", "mask", "sizes", "ret")

    def __init__(self, feat, topk, cost32, mask, sizes, ret):
        self.feat, self.topk, self.cost32, self.mask, self.sizes, self.ret = feat, topk, cost32, mask, sizes, ret


class RaggedPack:
    """A ragged batch on the device, as the C ABI takes it: C fp64, offsets (B,) int64, sizes and pos_off (B,)
    int32 (views of one uploaded block), posenc (rows, 8) f32, ld (0: packed), N, and the sizes on the host.
    offsets, sizes, pos_off and posenc are shared by every pack of the same sizes and layout: read-only."""
    __slots__ = ("C", "offsets", "sizes", "pos_off", "posenc", "ld", "N", "host_sizes")

    def __init__(self, C, offsets, sizes, pos_off, posenc, ld, N, host_sizes):
        self.C, self.offsets, self.sizes, self.pos_off, self.posenc = C, offsets, sizes, pos_off, posenc
        self.ld, self.N, self.host_sizes = ld, N, host_sizes


def _check_ragged_sizes(sizes, n_max=MAX_N):
    if len(sizes) < 1:
        raise ValueError("at least one cost matrix expected")
    if len(sizes) > MAX_BATCH:
        raise ValueError(f"at most {MAX_BATCH} instances per call, not {len(sizes)}")
    for n in sizes:
        if n < 1:
            raise ValueError("square, non-empty cost matrices expected")
        if n > n_max:
            raise ValueError(f"n exceeds the {n_max} limit of this call: {n}")


def ragged_pack(costs, device="cuda:0", sizes=None):
    """Host-side half of a ragged call: validates, packs and uploads.  `costs` is a sequence of square fp64
    matrices (NumPy: packed on the host into one buffer, one H2D copy; CUDA tensors: packed on the device), or,
    with `sizes`, one padded (B, N, N) fp64 array or CUDA tensor whose instance b is the prefix [:n_b, :n_b].
    Returns a RaggedPack.  Raises ValueError before any device work."""
    import torch
    if sizes is not None:
        shape = tuple(costs.shape)
        if len(shape) != 3 or shape[1] != shape[2]:
            raise ValueError(f"a padded batch must be (B, N, N), not {shape}")
        host_sizes = [int(n) for n in sizes]
        if len(host_sizes) != shape[0]:
            raise ValueError(f"{shape[0]} instances but {len(host_sizes)} sizes")
        N, ld = shape[1], shape[1]
        if N > MAX_N:
            raise ValueError(f"n exceeds the {MAX_N} limit of this build: {N}")
        _check_ragged_sizes(host_sizes, N)
        offsets = np.arange(len(host_sizes), dtype=np.int64) * (N * N)
        on_device = isinstance(costs, torch.Tensor) and costs.is_cuda
        mats = None
    else:
        mats = list(costs)
        on_device = bool(mats) and all(isinstance(c, torch.Tensor) and c.is_cuda for c in mats)
        if not on_device:
            mats = [np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c, dtype=np.float64) for c in mats]
        for c in mats:
            if c.ndim != 2 or c.shape[0] != c.shape[1]:
                raise ValueError(f"square cost matrices expected, not {tuple(c.shape)}")
            if on_device and c.dtype != torch.float64:
                raise ValueError("CUDA cost matrices must be float64")
        host_sizes = [int(c.shape[0]) for c in mats]
        _check_ragged_sizes(host_sizes)
        N, ld = max(host_sizes), 0
        sq = np.asarray(host_sizes, dtype=np.int64) ** 2
        offsets = np.concatenate(([0], np.cumsum(sq)[:-1])).astype(np.int64)
    if on_device and sizes is not None and costs.dtype != torch.float64:
        raise ValueError("a padded CUDA batch must be float64")
    _hip.require_device()
    device = torch.device(device)
    if sizes is not None:
        C = costs if on_device else torch.from_numpy(np.ascontiguousarray(costs, dtype=np.float64)).to(device)
        C = C.contiguous()
    elif on_device:
        device = mats[0].device
        C = torch.cat([c.reshape(-1) for c in mats])
    else:
        buf = np.empty(int(offsets[-1]) + host_sizes[-1] ** 2, dtype=np.float64)
        for c, o in zip(mats, offsets.tolist()):
            buf[o:o + c.size] = c.reshape(-1)
        C = torch.from_numpy(buf).to(device)
    offs_d, sizes_d, pos_off_d, posenc = _ragged_meta(tuple(host_sizes), ld, offsets, C.device)
    return RaggedPack(C, offs_d, sizes_d, pos_off_d, posenc, ld, N, host_sizes)


def row_features_ragged(costs, return_topk: bool = True, want_cost32: bool = False, device="cuda:0", sizes=None):
    """Row features of B cost matrices of different sizes in one call (two kernels): a RaggedFeatures padded to
    the largest size.  feat[b, :n_b] and topk[b, :n_b] are bit for bit what row_features_device gives for
    instance b alone; padded rows are 0 / +inf.  `costs`, `device`, `sizes`: see ragged_pack.  Enqueued on the
    current torch stream; nothing is read back."""
    return row_features_packed(ragged_pack(costs, device, sizes), return_topk, want_cost32)


def row_features_packed(pack: RaggedPack, return_topk: bool = True, want_cost32: bool = False):
    """row_features_ragged of a batch that is packed already."""
    import torch
    from ._call import hip_call
    lib = _hip.require_device()
    dev, B, N = pack.C.device, len(pack.host_sizes), pack.N
    feat = torch.empty((B, N, ROW_FEATURE_DIM), dtype=torch.float32, device=dev)
    topk = torch.empty((B, N, TOPK), dtype=torch.float32, device=dev) if return_topk else None
    cost32 = torch.empty((B, N, N), dtype=torch.float32, device=dev) if want_cost32 else None
    mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
    ret = torch.empty((B,), dtype=torch.int32, device=dev)
    ws_bytes = lib.lapwarm_ragged_workspace_bytes(B, N)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    hip_call("lapwarm_row_features_ragged", "row_features_ragged", dev, pack.C, pack.offsets, pack.sizes, pack.ld, B, N,
             pack.posenc, pack.pos_off, feat, topk, cost32, mask, ret, ws, ws_bytes)
    return RaggedFeatures(feat, topk, cost32, mask.view(torch.bool), pack.sizes, ret)


def min_trick_ragged(pack: RaggedPack, u=None):
    """v (B, N) f64 with v[b][j] = min_{i < n_b} (C_b[i][j] - u[b][i]) and 0 beyond n_b; u (B, N) f64 on the
    device, or None for the plain column minima."""
    import torch
    from ._call import hip_call
    lib = _hip.require_device()
    B, N, dev = len(pack.host_sizes), pack.N, pack.C.device
    if u is not None and (u.dtype != torch.float64 or tuple(u.shape) != (B, N) or not u.is_contiguous()):
        raise ValueError(f"u must be a contiguous float64 ({B}, {N}) tensor")
    v = torch.empty((B, N), dtype=torch.float64, device=dev)
    ws_bytes = lib.lapwarm_ragged_workspace_bytes(B, N)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    hip_call("lapwarm_colmin_ragged", "min_trick_ragged", dev, pack.C, pack.offsets, pack.sizes, pack.ld, B, N, u, v,
             ws, ws_bytes)
    return v


def _check_pack_vector(pack, name, t, optional=False):
    """Argument errors of a (B, N) fp64 device vector of a packed batch: type and dtype, then shape, then device."""
    import torch
    if t is None and optional:
        return
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"Argument '{name}' must be a torch.Tensor, not {type(t).__name__}")
    if t.dtype != torch.float64:
        raise TypeError(f"{name} must be torch.float64, not {t.dtype}")
    B, N = len(pack.host_sizes), pack.N
    if tuple(t.shape) != (B, N) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous ({B}, {N}) tensor, not {tuple(t.shape)}")
    if t.device != pack.C.device:
        raise ValueError(f"{name} must be on {pack.C.device} like the packed costs, not {t.device}")


def ragged_duals_workspace(pack):
    """The workspace of one call of the ragged dual utilities (lapwarm_ragged_duals_workspace_bytes)."""
    import torch
    nbytes = int(_hip.load().lapwarm_ragged_duals_workspace_bytes(len(pack.host_sizes), pack.N))
    return torch.empty((nbytes,), dtype=torch.uint8, device=pack.C.device), nbytes


def row_min_ragged(pack: RaggedPack, v=None):
    """out (B, N) f64 with out[b][i] = min_{j < n_b} (C_b[i][j] - v[b][j]) and 0 beyond n_b; v (B, N) f64 on the
    device, or None for the plain row minima.  One kernel on the current torch stream."""
    import torch
    from ._call import hip_call
    if not isinstance(pack, RaggedPack):
        raise TypeError(f"Argument 'pack' must be a RaggedPack, not {type(pack).__name__}")
    _check_pack_vector(pack, "v", v, optional=True)
    _hip.require_device()
    B, N, dev = len(pack.host_sizes), pack.N, pack.C.device
    out = torch.empty((B, N), dtype=torch.float64, device=dev)
    ws, ws_bytes = ragged_duals_workspace(pack)
    hip_call("lapwarm_rowmin_ragged", "row_min_ragged", dev, pack.C, pack.offsets, pack.sizes, pack.ld, B, N, v, out,
             None, ws, ws_bytes)
    return out


def compute_row_features_torch(cost):
    """Device-resident variant: CUDA tensor (n, n) of any float dtype -> (n, 21) float32 on the
    same device.  float32 inputs are widened exactly to float64 before the sweep."""
    import torch
    if cost.ndim != 2:
        raise ValueError("cost must be (n, m)")
    if cost.shape[0] == 0:
        return torch.zeros((0, 0), dtype=torch.float32, device=cost.device)
    if not cost.is_cuda:
        raise RuntimeError("compute_row_features_torch runs on the GPU only (no CPU fallback here)")
    return row_features_device(cost.to(torch.float64), return_topk=False)


def min_trick_device(C, u):
    """v[b][j] = min_i (C[b][i][j] - u[b][i]) in fp64 on the device (scripts/gnn_benchmark.py:262).
    C (B,n,n) f64 CUDA, u (B,n) any float dtype CUDA -> v (B,n) f64."""
    import torch
    from ._call import hip_call
    C = C.contiguous()
    B, n, _ = C.shape
    u64 = u.to(torch.float64).contiguous()
    lib = _hip.require_device()
    v = torch.empty((B, n), dtype=torch.float64, device=C.device)
    ws_bytes = lib.lapwarm_sweep_workspace_bytes(B, n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=C.device)
    hip_call("lapwarm_colmin_batched", "min_trick_device", C.device, C, B, n, u64, v, ws, ws_bytes)
    return v


@dataclass
class GraphFeatures:
    row_feat: np.ndarray
    col_feat: np.ndarray
    edge_feat: np.ndarray


def graph_features_device(C, u=None):
    """C (B, n, n) or (n, n) CUDA float64, u (B, n) or (n,) CUDA or None -> edge (B, n, n, 10), row (B, n, 14),
    col (B, n, 14), float32.  Channel 9 of edge is C - u - min_i(C - u) with u, 0 without.  Three kernels on the
    current torch stream; no host synchronisation."""
    import torch
    from ._call import hip_call
    if not C.is_cuda or C.dtype != torch.float64:
        raise TypeError("graph_features_device expects a CUDA float64 tensor")
    squeeze = C.ndim == 2
    if squeeze:
        C = C.unsqueeze(0)
    C = C.contiguous()
    B, n, m = C.shape
    if n != m or n < 1:
        raise ValueError("square, non-empty cost matrices expected")
    if n > GRAPH_MAX_N:
        raise ValueError(f"n exceeds the {GRAPH_MAX_N} limit of the graph features: {n}")
    if u is not None:
        u = u.to(device=C.device, dtype=torch.float64).reshape(B, n).contiguous()
    lib = _hip.require_device()
    edge = torch.empty((B, n, n, EDGE_FEATURE_DIM), dtype=torch.float32, device=C.device)
    row = torch.empty((B, n, NODE_FEATURE_DIM), dtype=torch.float32, device=C.device)
    col = torch.empty((B, n, NODE_FEATURE_DIM), dtype=torch.float32, device=C.device)
    ws_bytes = int(lib.lapwarm_graph_features_workspace_bytes(B, n))
    if ws_bytes == 0:
        raise ValueError(f"graph_features_device: batch {B} or n {n} out of range")
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=C.device)
    pos = _posenc_device(n, C.device)
    hip_call("lapwarm_graph_features_batched", "graph_features_device", C.device, C, B, n, u, pos, edge, row, col, ws,
             ws_bytes)
    if squeeze:
        edge, row, col = edge[0], row[0], col[0]
    return edge, row, col


class RaggedGraphFeatures:
    """What one ragged graph-feature call returns, padded to N = the largest size: edge (B, N, N, 10), row and col
    (B, N, 14) f32, 0 outside every prefix, mask (B, N) bool, sizes (B,) int32 and ret (B,) int32 (0, or 2 for a
    size outside 1..N), all on the device."""
    __slots__ = ("edge", "row", "col", "mask", "sizes", "ret")

    def __init__(self, edge, row, col, mask, sizes, ret):
        self.edge, self.row, self.col, self.mask, self.sizes, self.ret = edge, row, col, mask, sizes, ret


def graph_features_ragged(costs, u=None, device="cuda:0", sizes=None):
    """DualGNN's graph features of B cost matrices of different sizes in one call (three kernels): a
    RaggedGraphFeatures padded to the largest size.  edge[b, :n_b, :n_b], row[b, :n_b] and col[b, :n_b] are bit for
    bit what graph_features_device gives instance b alone; everything else is 0, as the reference's collate
    (gnn/train.py) pads.  `costs`, `device`, `sizes`: see ragged_pack; u: (B, N) float64 on the device, read on each
    prefix, or None.  Enqueued on the current torch stream; nothing is read back."""
    if sizes is None:
        costs = list(costs)
        width = max((int(np.shape(c)[0]) for c in costs if np.ndim(c) == 2), default=0)
    else:
        width = int(costs.shape[1]) if len(costs.shape) == 3 else 0
    if width > GRAPH_MAX_N:
        raise ValueError(f"n exceeds the {GRAPH_MAX_N} limit of the graph features: {width}")
    return graph_features_packed(ragged_pack(costs, device, sizes), u)


def graph_features_packed(pack: RaggedPack, u=None):
    """graph_features_ragged of a batch that is packed already."""
    import torch
    from ._call import hip_call
    B, N, dev = len(pack.host_sizes), pack.N, pack.C.device
    if N > GRAPH_MAX_N:
        raise ValueError(f"n exceeds the {GRAPH_MAX_N} limit of the graph features: {N}")
    _check_pack_vector(pack, "u", u, optional=True)
    lib = _hip.require_device()
    ws_bytes = int(lib.lapwarm_graph_features_ragged_workspace_bytes(B, N))
    if ws_bytes == 0:
        raise ValueError(f"graph_features_packed: batch {B} or N {N} out of range")
    edge = torch.empty((B, N, N, EDGE_FEATURE_DIM), dtype=torch.float32, device=dev)
    row = torch.empty((B, N, NODE_FEATURE_DIM), dtype=torch.float32, device=dev)
    col = torch.empty((B, N, NODE_FEATURE_DIM), dtype=torch.float32, device=dev)
    mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
    ret = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    hip_call("lapwarm_graph_features_ragged", "graph_features_ragged", dev, pack.C, pack.offsets, pack.sizes, pack.ld,
             B, N, u, pack.posenc, pack.pos_off, edge, row, col, mask, ret, ws, ws_bytes)
    return RaggedGraphFeatures(edge, row, col, mask.view(torch.bool), pack.sizes, ret)


def compute_features(C: np.ndarray, *, include_reduced_cost: bool = False, u=None) -> GraphFeatures:
    """The reference's compute_features (gnn/features.py:49-153): float64 (n, n) NumPy in, GraphFeatures of
    float32 NumPy out; the work happens on the GPU."""
    import torch
    C = np.ascontiguousarray(np.asarray(C, dtype=np.float64))
    if C.ndim != 2 or C.shape[0] != C.shape[1] or C.shape[0] < 1:
        raise ValueError("compute_features on the MI355X path expects a square, non-empty cost matrix")
    _hip.require_device()
    Cd = torch.from_numpy(C).to("cuda:0")
    ud = None
    if include_reduced_cost and u is not None:
        ud = torch.from_numpy(np.ascontiguousarray(np.asarray(u, dtype=np.float64))).to("cuda:0")
    edge, row, col = graph_features_device(Cd, ud)
    return GraphFeatures(row_feat=row.cpu().numpy(), col_feat=col.cpu().numpy(), edge_feat=edge.cpu().numpy())
