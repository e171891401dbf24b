"""Warm-start pipeline on the MI355X: C -> row features -> OneGNN u -> v = min(C - u) ->
lapjv_seeded(C, u, v), batched over independent cost matrices that stay resident in HBM.

Two entry points:
  * `GNNPredictor` -- the harness-facing object of the reference (scripts/gnn_benchmark.py:56-289):
    `GNNPredictor(model_path).predict(C) -> (u, v)` with float64 NumPy in/out;
  * `WarmStartPipeline` -- the batched device API: torch CUDA tensors
    in/out, everything enqueued on the current stream, no host round trips between stages.
"""
from __future__ import annotations

import ctypes as ct
from collections.abc import Sequence
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import torch

from lap import _hip
from ._call import hip_call
from .dual_gnn import DualGNN
from .features import (ROW_FEATURE_DIM, RaggedPack, _check_pack_vector, graph_features_device,
                       graph_features_packed, min_trick_device, min_trick_ragged, ragged_pack, row_features_device, row_features_packed, row_min_ragged)
from .one_gnn import OneGNN

STATS_FIELDS = ("branch", "tight_edges", "free_rows", "arr_fired", "paths", "finds", "scan_steps",
                "scan_elems", "init_elems", "colred_elems", "transfer_rows", "arr_iters", "err",
                "r13", "r14", "r15")


def load_checkpoint(path, device="cpu") -> Tuple[OneGNN, dict]:
    """Build a OneGNN from a reference checkpoint.  Both schemas are accepted: flat
    (gnn/train_one_gnn.py:409-420) and nested under 'config'
    (gnn/train_progressive_clean.py:601-608); merged as scripts/gnn_benchmark.py:80-119 does.
    Files are read with weights_only=True (nothing in them is executed)."""
    ckpt = torch.load(str(path), map_location=device, weights_only=True)
    if isinstance(ckpt, dict) and "model_state_dict" in ckpt:
        state = ckpt["model_state_dict"]
        info = {
            "architecture": ckpt.get("architecture", "dual_gnn"),
            "hidden_dim": ckpt.get("hidden_dim", 128),
            "layers": ckpt.get("layers", 4),
            "dropout": ckpt.get("dropout", 0.1),
            "row_feat_dim": ckpt.get("row_feat_dim"),
        }
        cfg = ckpt.get("config")
        if isinstance(cfg, dict):
            for k in info:
                info[k] = cfg.get(k, info[k])
    else:
        raise ValueError("bare state dicts are legacy DualGNN checkpoints; only OneGNN is on the hot path")
    if info["architecture"] != "one_gnn":
        raise ValueError(f"architecture '{info['architecture']}' is not on the warm-start hot path (OneGNN only)")
    in_dim = info.get("row_feat_dim") or ROW_FEATURE_DIM
    if in_dim != ROW_FEATURE_DIM:
        raise ValueError(f"Checkpoint expects {in_dim} row features but the pipeline now uses {ROW_FEATURE_DIM}.")
    model = OneGNN(in_dim=in_dim, hidden=info["hidden_dim"], layers=info["layers"], dropout=info["dropout"])
    model.load_state_dict(state)
    model.to(device).eval()
    return model, info


def load_dual_checkpoint(path, device="cpu") -> Tuple[DualGNN, dict]:
    """Build a DualGNN from a reference checkpoint, as scripts/gnn_benchmark.py:80-119 reads it.  A bare state
    dict is a legacy DualGNN checkpoint: hidden 128, 4 layers, 4 heads, dropout 0.1.  The flat schema and the one
    nested under 'config' are accepted with architecture == "dual_gnn" (the default of a file that names none),
    `heads` included.  Files are read with weights_only=True."""
    ckpt = torch.load(str(path), map_location=device, weights_only=True)
    info = {"architecture": "dual_gnn", "hidden_dim": 128, "layers": 4, "heads": 4, "dropout": 0.1}
    if isinstance(ckpt, dict) and "model_state_dict" in ckpt:
        state = ckpt["model_state_dict"]
        cfg = ckpt.get("config")
        for k in info:
            info[k] = ckpt.get(k, info[k])
            if isinstance(cfg, dict):
                info[k] = cfg.get(k, info[k])
    elif isinstance(ckpt, dict):
        state = ckpt
    else:
        raise ValueError(f"not a checkpoint: {type(ckpt).__name__}")
    if info["architecture"] != "dual_gnn":
        raise ValueError(f"architecture '{info['architecture']}' is not DualGNN; use load_checkpoint")
    model = DualGNN(hidden_dim=info["hidden_dim"], layers=info["layers"], heads=info["heads"],
                    dropout=info["dropout"])
    model.load_state_dict(state)
    model.to(device).eval()
    return model, info


def _check_rounds(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"Argument '{name}' must be an int, not {type(value).__name__}")
    if not -2**31 <= value < 2**31:
        raise ValueError(f"{name} must fit an int32, not {value}")
    return int(value)


def _check_real(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise TypeError(f"Argument '{name}' must be a float, not {type(value).__name__}")
    return float(value)


def _check_noise_args(std, prob, generator, names):
    """(std, prob) as floats: types first, then values; `generator` a torch.Generator or None."""
    std, prob = _check_real(std, names[0]), _check_real(prob, names[1])
    if generator is not None and not isinstance(generator, torch.Generator):
        raise TypeError(f"Argument 'generator' must be a torch.Generator, not {type(generator).__name__}")
    if not std >= 0.0:
        raise ValueError(f"{names[0]} must be >= 0, not {std}")
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"{names[1]} must be in [0, 1], not {prob}")
    return std, prob


class RaggedDuals(Sequence):
    """What oracle_duals_many returns: entry b is (x, u, v, ret, sweeps) of instance b, sliced to n_b.  The
    entries are views of the padded device tensors x, u, v (B, N), ret (B,) and sweeps (B, 4), which are the
    fields; a view is made when its entry is read, so a caller that wants the padded batch pays for none."""
    __slots__ = ("x", "u", "v", "ret", "sweeps", "sizes")

    def __init__(self, x, u, v, ret, sweeps, sizes):
        self.x, self.u, self.v, self.ret, self.sweeps, self.sizes = x, u, v, ret, sweeps, sizes

    def __len__(self):
        return len(self.sizes)

    def __getitem__(self, b):
        if isinstance(b, slice):
            return [self[k] for k in range(*b.indices(len(self)))]
        n = self.sizes[b]  # (IndexError ends an iteration)
        return self.x[b, :n], self.u[b, :n], self.v[b, :n], self.ret[b], self.sweeps[b]


NONSQUARE = "Square cost array expected. If cost is intentionally non-square, pass extend_cost=True."


class ExtendedPack:
    """A batch of cost matrices of different shapes on the device, as lapwarm_lapjv_extended_ragged takes it:
    C fp64 (flat), offsets (B,) int64, limits (B,) fp64, rows and cols (B,) int32 (views of one uploaded block),
    ld (0: packed), and the shapes and limits on the host."""
    __slots__ = ("C", "offsets", "limits", "rows", "cols", "ld", "host_rows", "host_cols", "host_limits")

    def __init__(self, C, offsets, limits, rows, cols, ld, host_rows, host_cols, host_limits):
        self.C, self.offsets, self.limits, self.rows, self.cols, self.ld = C, offsets, limits, rows, cols, ld
        self.host_rows, self.host_cols, self.host_limits = host_rows, host_cols, host_limits


def _extended_meta(offsets, host_rows, host_cols, host_limits, device):
    """offsets, limits, rows, cols on the device from one host block and one copy."""
    B = len(host_rows)
    block = np.empty((24 * B,), dtype=np.uint8)
    block[:8 * B].view(np.int64)[:] = offsets
    block[8 * B:16 * B].view(np.float64)[:] = host_limits
    block[16 * B:20 * B].view(np.int32)[:] = host_rows
    block[20 * B:].view(np.int32)[:] = host_cols
    d = torch.from_numpy(block).to(device)
    return (d[:8 * B].view(torch.int64), d[8 * B:16 * B].view(torch.float64), d[16 * B:20 * B].view(torch.int32),
            d[20 * B:].view(torch.int32))


def _limits_of(cost_limit, count):
    """One fp64 limit per instance from a scalar or a sequence of `count` values."""
    if np.ndim(cost_limit) == 0:
        return [float(cost_limit)] * count
    limits = [float(t) for t in cost_limit]
    if len(limits) != count:
        raise ValueError(f"{count} cost matrices but {len(limits)} cost limits")
    return limits


def extended_pack(costs, cost_limit=float("inf"), device="cuda:0") -> ExtendedPack:
    """Host-side half of a ragged lapjv_extended call: `costs` is a sequence of non-empty 2-D fp64 matrices
    (NumPy: packed on the host, one H2D copy; CUDA tensors: packed on the device), `cost_limit` a scalar or one
    value per instance.  Raises before any device work."""
    mats = list(costs)
    if not mats:
        raise ValueError("at least one cost matrix expected")
    on_device = all(isinstance(c, torch.Tensor) and c.is_cuda for c in mats)
    if not on_device:
        mats = [np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c) for c in mats]
    for c in mats:
        if c.ndim != 2:
            raise ValueError("2-dimensional array expected")
        if on_device and c.dtype != torch.float64:
            raise ValueError("CUDA cost matrices must be float64")
        if c.shape[0] < 1 or c.shape[1] < 1:
            raise ValueError("non-empty cost matrices expected")
    host_limits = _limits_of(cost_limit, len(mats))
    host_rows, host_cols = [int(c.shape[0]) for c in mats], [int(c.shape[1]) for c in mats]
    counts = np.asarray(host_rows, dtype=np.int64) * np.asarray(host_cols, dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum(counts)[:-1])).astype(np.int64)
    _hip.require_device()
    if on_device:
        device = mats[0].device
        C = torch.cat([c.reshape(-1) for c in mats])
    else:
        buf = np.empty(int(counts.sum()), dtype=np.float64)
        for c, o in zip(mats, offsets.tolist()):
            buf[o:o + c.size] = np.asarray(c, dtype=np.float64).reshape(-1)
        C = torch.from_numpy(buf).to(torch.device(device))
    offs_d, lim_d, rows_d, cols_d = _extended_meta(offsets, host_rows, host_cols, host_limits, C.device)
    return ExtendedPack(C, offs_d, lim_d, rows_d, cols_d, 0, host_rows, host_cols, host_limits)


class SparsePack:
    """A batch of CSR problems on the device, as lapwarm_lapmod_ragged takes it: cc fp64 and kk int32 (all entries,
    one instance behind the other), ii int32 (n_b + 1 local row starts per instance), nnz_offsets, row_offsets (B,)
    int64 and sizes (B,) int32, and the sizes and entry counts on the host."""
    __slots__ = ("cc", "kk", "ii", "nnz_offsets", "row_offsets", "sizes", "host_sizes", "host_nnz")

    def __init__(self, cc, kk, ii, nnz_offsets, row_offsets, sizes, host_sizes, host_nnz):
        self.cc, self.kk, self.ii = cc, kk, ii
        self.nnz_offsets, self.row_offsets, self.sizes = nnz_offsets, row_offsets, sizes
        self.host_sizes, self.host_nnz = host_sizes, host_nnz


def sparse_pack(problems, device="cuda:0") -> SparsePack:
    """Host-side half of a lapmod_ragged call: `problems` is a sequence of (n, cc, ii, kk) (lap._lapmod checks
    them); everything is packed into one host block and copied once."""
    probs = [(int(n), np.ascontiguousarray(cc, dtype=np.float64), np.ascontiguousarray(ii, dtype=np.int32),
              np.ascontiguousarray(kk, dtype=np.int32)) for n, cc, ii, kk in problems]
    if not probs:
        raise ValueError("at least one problem expected")
    for n, cc, ii, kk in probs:
        if n < 1 or ii.shape != (n + 1,) or cc.ndim != 1 or cc.shape != kk.shape or int(ii[-1]) != cc.size:
            raise ValueError("sparse_pack: (n, cc, ii, kk) with len(ii) == n + 1 and ii[n] == len(cc) == len(kk)")
        if cc.size >= 2 ** 31:
            raise ValueError("sparse_pack: an instance must have fewer than 2**31 entries (ii is int32)")
    B = len(probs)
    host_sizes = [p[0] for p in probs]
    host_nnz = [int(p[1].size) for p in probs]
    nnz_off = np.concatenate(([0], np.cumsum(host_nnz)[:-1])).astype(np.int64)
    row_off = np.concatenate(([0], np.cumsum([n + 1 for n in host_sizes])[:-1])).astype(np.int64)
    total, rows = int(sum(host_nnz)), int(sum(host_sizes)) + B
    o_kk = 8 * total
    o_ii = o_kk + 4 * total
    o_meta = (o_ii + 4 * rows + 7) & ~7
    block = np.zeros((o_meta + 20 * B,), dtype=np.uint8)
    block[:o_kk].view(np.float64)[:] = np.concatenate([p[1] for p in probs])
    block[o_kk:o_ii].view(np.int32)[:] = np.concatenate([p[3] for p in probs])
    block[o_ii:o_ii + 4 * rows].view(np.int32)[:] = np.concatenate([p[2] for p in probs])
    block[o_meta:o_meta + 8 * B].view(np.int64)[:] = nnz_off
    block[o_meta + 8 * B:o_meta + 16 * B].view(np.int64)[:] = row_off
    block[o_meta + 16 * B:].view(np.int32)[:] = host_sizes
    _hip.require_device()
    d = torch.from_numpy(block).to(torch.device(device))
    return SparsePack(d[:o_kk].view(torch.float64), d[o_kk:o_ii].view(torch.int32),
                      d[o_ii:o_ii + 4 * rows].view(torch.int32), d[o_meta:o_meta + 8 * B].view(torch.int64),
                      d[o_meta + 8 * B:o_meta + 16 * B].view(torch.int64), d[o_meta + 16 * B:].view(torch.int32),
                      host_sizes, host_nnz)


def _solve_outputs(B, width, index_dtype, device, want_stats, ragged=False):
    """What a solve writes: x, y (B, width) of `index_dtype`, ret (B,) int32 and stats (B, 32) int64 or None.
    The stats of a uniform batch start at zero; the first kernel of a ragged call initialises its own."""
    x = torch.empty((B, width), dtype=index_dtype, device=device)
    y = torch.empty((B, width), dtype=index_dtype, device=device)
    ret = torch.empty((B,), dtype=torch.int32, device=device)
    stats = (torch.empty if ragged else torch.zeros)((B, 32), dtype=torch.int64, device=device) if want_stats else None
    return x, y, ret, stats


class WarmStartPipeline:
    """Batched, device-resident warm-start solve."""

    def __init__(self, model: OneGNN, device="cuda:0", threads_hint: int = 0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("WarmStartPipeline runs on the MI355X only")
        self.lib = _hip.require_device()
        self.model = model.to(self.device).eval()
        self.threads_hint = int(threads_hint)
        self._ws = {}
        self._ragged_ok = {}  # size -> does seeded_ragged take it
        self._cold_ragged_ok = {}  # size -> does lapjv_ragged take it

    def _workspace(self, B, n, cold=False):
        # (cold solves carry the candidate lists of the row reduction: a larger block, cached separately)
        query = self.lib.lapwarm_lapjv_workspace_bytes if cold else self.lib.lapwarm_seeded_workspace_bytes
        return self._cached_workspace((B, n, cold), lambda: query(B, n))

    def _cached_workspace(self, key, nbytes_of):
        if key not in self._ws:
            if len(self._ws) >= 4:  # a handful of shapes at most: drop the oldest
                # kernels of an earlier call may still be running on it (any stream), and a captured
                # graph may hold its address: wait for the device before the block can be handed out again
                torch.cuda.synchronize(self.device)
                self._ws.pop(next(iter(self._ws)))
            nbytes = int(nbytes_of())
            self._ws[key] = (torch.empty((nbytes,), dtype=torch.uint8, device=self.device), nbytes)
        ws = self._ws[key]
        # the caching allocator must not recycle the block while the stream that uses it now still runs
        ws[0].record_stream(torch.cuda.current_stream(self.device))
        return ws

    @torch.inference_mode()
    def predict_batch(self, C: torch.Tensor):
        """C (B,n,n) f64 CUDA -> u (B,n) f32 (the model output), v (B,n) f64 (fp64 min-trick on
        the float64-widened u, as the reference's CPU branch does)."""
        feat, topk = row_features_device(C)
        mask = torch.ones(feat.shape[:2], dtype=torch.bool, device=C.device)
        u = self.model(feat, mask=mask, topk_values=topk)["u"]
        v = min_trick_device(C, u)
        return u, v

    def seeded_batch(self, C: torch.Tensor, u: torch.Tensor, v: torch.Tensor, eps: float = 1e-12,
                     want_stats: bool = True):
        """Batched lapjv_seeded: x, y (B,n) int64, ret (B,) int32, stats (B,32) int64."""
        C = C.contiguous()
        B, n, _ = C.shape
        u = u.to(torch.float64).contiguous()
        v = v.to(torch.float64).contiguous()
        x, y, ret, stats = _solve_outputs(B, n, torch.int64, C.device, want_stats)
        ws, nbytes = self._workspace(B, n)
        hip_call("lapwarm_seeded_batched", "seeded_batch", C.device, C, B, n, u, v, float(eps), x, y, ret, stats, ws,
                 nbytes, self.threads_hint)
        return x, y, ret, stats

    def lapjv_batch(self, C: torch.Tensor, want_stats: bool = True):
        """Batched cold lapjv: x, y (B,n) int32, ret (B,), stats."""
        C = C.contiguous()
        B, n, _ = C.shape
        x, y, ret, stats = _solve_outputs(B, n, torch.int32, C.device, want_stats)
        ws, nbytes = self._workspace(B, n, cold=True)
        hip_call("lapwarm_lapjv_batched", "lapjv_batch", C.device, C, B, n, x, y, ret, stats, ws, nbytes,
                 self.threads_hint)
        return x, y, ret, stats

    def lapjv_extended_batch(self, C: torch.Tensor, extend_cost: bool = True, cost_limit: float = float("inf"),
                             want_stats: bool = True) -> dict:
        """Batched rectangular / cost-limited lapjv (the reference's `lapjv(cost, extend_cost, cost_limit)`,
        LAP/_lapjv_cpp/_lapjv.pyx:77-124) of a resident batch of one shape: C (B, n_rows, n_cols) fp64.
        Returns x (B, n_rows), y (B, n_cols) int32 with -1 for unmatched, opt (B,) fp64, matched (B,) int32,
        ret (B,) int32 and stats (B, 32) int64 of the cold solve of the square problem (or None).  The
        extended matrices are built in the workspace on the device; everything is enqueued on the current
        stream."""
        if C.dim() != 3 or C.dtype != torch.float64 or not C.is_cuda:
            raise ValueError("C must be a (B, n_rows, n_cols) float64 CUDA tensor")
        C = C.contiguous()
        B, n_rows, n_cols = C.shape
        extend_cost, cost_limit = int(bool(extend_cost)), float(cost_limit)
        n = self.lib.lapwarm_lapjv_extended_n(n_rows, n_cols, extend_cost, cost_limit)
        if n == -4:
            raise ValueError(NONSQUARE)
        if n == -2 or B < 1:
            raise ValueError("lapjv_extended_batch: empty batch or empty cost matrices")
        _hip.check(n, "lapjv_extended_batch")
        x = torch.empty((B, n_rows), dtype=torch.int32, device=C.device)
        y = torch.empty((B, n_cols), dtype=torch.int32, device=C.device)
        opt = torch.empty((B,), dtype=torch.float64, device=C.device)
        matched = torch.empty((B,), dtype=torch.int32, device=C.device)
        ret = torch.empty((B,), dtype=torch.int32, device=C.device)
        stats = torch.zeros((B, 32), dtype=torch.int64, device=C.device) if want_stats else None
        ws, nbytes = self._cached_workspace(
            ("extended", B, n_rows, n_cols, extend_cost, cost_limit < float("inf")),
            lambda: self.lib.lapwarm_lapjv_extended_workspace_bytes(B, n_rows, n_cols, extend_cost, cost_limit))
        hip_call("lapwarm_lapjv_extended_batched", "lapjv_extended_batch", C.device, C, B, n_rows, n_cols, extend_cost,
                 cost_limit, x, y, opt, matched, ret, stats, ws, nbytes, self.threads_hint)
        return {"x": x, "y": y, "opt": opt, "matched": matched, "ret": ret, "stats": stats}

    def lapjv_ragged_eligible(self, n: int) -> bool:
        """Does lapjv_ragged take an instance of this size?  Those whose own cold plan is one launch with all
        solver state in LDS and no candidate lists: every n <= 511 with the default settings (the library
        decides, from the plan)."""
        known = self._cold_ragged_ok
        if n not in known:
            one = (ct.c_int * 1)(int(n))
            known[n] = self.lib.lapwarm_lapjv_ragged_groups(one, 1, (ct.c_int * 1)()) == 1
        return known[n]

    def lapjv_ragged(self, pack: RaggedPack, want_stats: bool = True):
        """Cold lapjv of every instance of a ragged batch in one call (lapwarm_lapjv_ragged): one solver launch
        per kernel configuration, `pack.C` read where it is.  Returns x, y (B, N) int64 with -1 beyond n_b, ret
        (B,) int32, stats (B, 32) int64 or None; row b is what lapjv_batch gives instance b alone with
        threads_hint 0 (x, y as int64).  Every size must be in the class `lapjv_ragged_eligible` describes."""
        if not isinstance(pack, RaggedPack):
            raise TypeError(f"Argument 'pack' must be a RaggedPack, not {type(pack).__name__}")
        B, N, dev = len(pack.host_sizes), pack.N, pack.C.device
        x, y, ret, stats = _solve_outputs(B, N, torch.int64, dev, want_stats, ragged=True)
        ws, nbytes = self._cached_workspace(("lapjv_ragged", B, N),
                                            lambda: self.lib.lapwarm_lapjv_ragged_workspace_bytes(B, N))
        host_sizes = (ct.c_int * B)(*pack.host_sizes)
        hip_call("lapwarm_lapjv_ragged", "lapjv_ragged", dev, pack.C, pack.offsets, pack.sizes, host_sizes, pack.ld, B,
                 N, x, y, ret, stats, ws, nbytes)
        return x, y, ret, stats

    def lapjv_extended_ragged(self, pack: ExtendedPack, extend_cost: bool = True, want_stats: bool = True) -> dict:
        """lapjv_extended_batch for instances of different shapes and limits in one call
        (lapwarm_lapjv_extended_ragged): `pack` is an extended_pack result.  Returns the same dict, padded: x
        (B, R), y (B, Q) int32 with -1 for unmatched and beyond the instance's shape (R, Q the largest n_rows,
        n_cols), opt (B,) fp64, matched, ret (B,) int32 and stats (B, 32) int64 or None; row b is what
        lapjv_extended_batch gives instance b alone.  Every extended size must be in the class
        `lapjv_ragged_eligible` describes."""
        if not isinstance(pack, ExtendedPack):
            raise TypeError(f"Argument 'pack' must be an ExtendedPack, not {type(pack).__name__}")
        B, dev, extend_cost = len(pack.host_rows), pack.C.device, int(bool(extend_cost))
        rows, cols = (ct.c_int * B)(*pack.host_rows), (ct.c_int * B)(*pack.host_cols)
        limits = (ct.c_double * B)(*pack.host_limits)
        R, Q = max(pack.host_rows), max(pack.host_cols)
        nbytes = int(self.lib.lapwarm_lapjv_extended_ragged_workspace_bytes(rows, cols, limits, extend_cost, B))
        if nbytes == 0:
            for r, c, t in zip(pack.host_rows, pack.host_cols, pack.host_limits):
                n = self.lib.lapwarm_lapjv_extended_n(r, c, extend_cost, t)
                if n == -4:
                    raise ValueError(NONSQUARE)
                _hip.check(n, "lapjv_extended_ragged")
            raise ValueError("lapjv_extended_ragged: empty batch or empty cost matrices")
        x = torch.empty((B, R), dtype=torch.int32, device=dev)
        y = torch.empty((B, Q), dtype=torch.int32, device=dev)
        opt = torch.empty((B,), dtype=torch.float64, device=dev)
        matched = torch.empty((B,), dtype=torch.int32, device=dev)
        ret = torch.empty((B,), dtype=torch.int32, device=dev)
        stats = torch.empty((B, 32), dtype=torch.int64, device=dev) if want_stats else None
        # (one block per power of two of the size: the shapes of a tracker change with every call)
        bucket = max(1 << 16, 1 << (nbytes - 1).bit_length())
        ws, cap = self._cached_workspace(("extended_ragged", bucket), lambda: bucket)
        hip_call("lapwarm_lapjv_extended_ragged", "lapjv_extended_ragged", dev, pack.C, pack.offsets, pack.rows,
                 pack.cols, pack.limits, rows, cols, limits, pack.ld, extend_cost, B, R, Q, x, y, opt, matched, ret,
                 stats, ws, cap)
        return {"x": x, "y": y, "opt": opt, "matched": matched, "ret": ret, "stats": stats}

    def lapmod_ragged(self, pack: SparsePack, fp_version: int = 3, want_stats: bool = True) -> dict:
        """Sparse LAPMOD of every instance of a SparsePack in one call (lapwarm_lapmod_ragged), inputs read where
        they are.  Returns x, y (B, N) int32 with -1 beyond n_b, v (B, N) fp64 (the final column duals, NaN beyond
        n_b and where ret != 0), ret (B,) int32 (0 solved, 1 no perfect matching: x, y -1) and stats (B, 32) int64
        or None.  Everything is enqueued on the current stream."""
        if not isinstance(pack, SparsePack):
            raise TypeError(f"Argument 'pack' must be a SparsePack, not {type(pack).__name__}")
        if isinstance(fp_version, bool) or not isinstance(fp_version, (int, np.integer)) or not 1 <= fp_version <= 3:
            raise ValueError(f"fp_version must be FP_1, FP_2 or FP_DYNAMIC (1, 2, 3), not {fp_version!r}")
        B, N, dev = len(pack.host_sizes), max(pack.host_sizes), pack.cc.device
        host_sizes = (ct.c_int * B)(*pack.host_sizes)
        host_nnz = (ct.c_longlong * B)(*pack.host_nnz)
        nbytes = int(self.lib.lapwarm_lapmod_workspace_bytes(host_sizes, host_nnz, B))
        if nbytes == 0:
            raise ValueError("lapmod_ragged: a batch of 1..65535 instances with 1 <= n <= 65535 expected")
        x, y, ret, stats = _solve_outputs(B, N, torch.int32, dev, want_stats, ragged=True)
        v = torch.empty((B, N), dtype=torch.float64, device=dev)
        bucket = max(1 << 16, 1 << (nbytes - 1).bit_length())
        ws, cap = self._cached_workspace(("lapmod_ragged", bucket), lambda: bucket)
        hip_call("lapwarm_lapmod_ragged", "lapmod_ragged", dev, pack.cc, pack.kk, pack.ii, pack.nnz_offsets,
                 pack.row_offsets, pack.sizes, host_sizes, B, N, int(fp_version), x, y, v, ret, stats, ws, cap)
        return {"x": x, "y": y, "v": v, "ret": ret, "stats": stats}

    # ---- exact dense solve through sparse LAPMOD (csrc/prune_price.hip; DESIGN.md, "Exact dense LAP through sparse
    # LAPMOD"): prune the dense rows to CSR, solve, price the absent entries with the duals, grow, repeat
    def prune_grow(self, pack: RaggedPack, m: int, key=None, x=None, csr: Optional[SparsePack] = None,
                   write: bool = True):
        """One grow step (lapwarm_prune_grow_ragged).  key (B, N) fp64 or None, x (B, N) int32 or None, csr the
        current CSR (a SparsePack over the same instances) or None for the diagonal.  Returns (next, counts): next
        a SparsePack without host_nnz (None without `write`: a pricing step), counts an int64 device block with
        added [:B], viol [B:2B] and, as int32, ret [2B:]; `prune_counts` reads it back."""
        B, N, dev = len(pack.host_sizes), pack.N, pack.C.device
        sizes = pack.host_sizes
        counts = torch.empty((2 * B + (B + 1) // 2,), dtype=torch.int64, device=dev)
        added, viol, ret = counts[:B], counts[B:2 * B], counts[2 * B:].view(torch.int32)
        need = int(self.lib.lapwarm_prune_workspace_bytes(B, N))
        if need == 0:
            raise ValueError("prune_grow: a batch of 1..65535 instances with 1 <= n <= 16384 expected")
        # (one block per power of two of the size: the live set shrinks from round to round)
        bucket = max(1 << 16, 1 << (need - 1).bit_length())
        ws, nbytes = self._cached_workspace(("prune", bucket), lambda: bucket)
        nxt = None
        out = [None] * 6
        if write:
            # what an instance can hold after the step: known without a read-back
            if csr is None:
                cap = [n * min(m + 1, n) for n in sizes]
            else:
                cap = [min(nz + n * m, n * n) for n, nz in zip(sizes, csr.host_nnz)]
            meta = np.empty((3, B), dtype=np.int64)
            meta[0] = np.concatenate(([0], np.cumsum(cap)[:-1]))
            meta[1] = np.concatenate(([0], np.cumsum([n + 1 for n in sizes])[:-1]))
            meta[2] = cap
            meta_d = torch.from_numpy(meta).to(dev)
            total, rows = int(sum(cap)), int(sum(sizes)) + B
            nxt = SparsePack(torch.empty((total,), dtype=torch.float64, device=dev),
                             torch.empty((total,), dtype=torch.int32, device=dev),
                             torch.empty((rows,), dtype=torch.int32, device=dev), meta_d[0], meta_d[1], pack.sizes,
                             sizes, None)
            out = [nxt.cc, nxt.kk, nxt.ii, meta_d[0], meta_d[1], meta_d[2]]
        cur = [None] * 4 if csr is None else [csr.kk, csr.ii, csr.nnz_offsets, csr.row_offsets]
        hip_call("lapwarm_prune_grow_ragged", "prune_grow", dev, pack.C, pack.offsets, pack.sizes, pack.ld, B, N, key,
                 x, *cur, int(m), *out, added, viol, ret, ws, nbytes)
        return nxt, counts

    @staticmethod
    def prune_counts(counts, B, *more):
        """[added, viol, ret] of a grow step over B instances as host lists, and every (B,) int32 tensor of `more`
        likewise: one copy, one synchronisation."""
        host = torch.cat([counts] + [t.to(torch.int64) for t in more]).cpu().numpy()
        res = [host[:B].tolist(), host[B:2 * B].tolist(), host[2 * B:counts.numel()].view(np.int32)[:B].tolist()]
        for q in range(len(more)):
            res.append(host[counts.numel() + q * B:counts.numel() + (q + 1) * B].tolist())
        return res

    def lapjv_pruned_ragged(self, pack: RaggedPack, k: int = 16, seed=None, max_rounds: int = 32) -> dict:
        """Exact lapjv of every instance of a ragged batch through sparse LAPMOD.  Round 0 keeps, per row, the
        diagonal and the k columns with the smallest C_ij - seed_j (ties to the lower column); lapmod_ragged
        (FP_DYNAMIC) solves the CSR; the pricing step adds to row i the at most k absent columns with the smallest
        C_ij - v_j among those below u_i = C[i][x_i] - v[x_i]; an instance without such a column is certified
        optimal and leaves the loop (the live instances are compacted on the host, so a certified one costs nothing
        afterwards).  seed (B, N) fp64 on the device or None.  Returns device tensors: x, y (B, N) int32 (-1 beyond
        n_b), u, v (B, N) fp64 (0 beyond n_b), cost (B,) fp64 (the sum of C[i][x_i] in ascending i), ret (B,) int32
        (0 certified; 2 not certified after max_rounds solves: x, y are the last solve's; 3 not admissible -- a cost
        outside [0, 1e6), NaN, or a seed that is not finite: x, y -1 and cost inf, nothing solved; 4 treated as
        empty), rounds (B,) int32 the solves run, nnz (B,) int64 the size of the last CSR solved and viol_last (B,)
        int64 (0 exactly when certified).  One small read-back per round: not graph-capturable."""
        if not isinstance(pack, RaggedPack):
            raise TypeError(f"Argument 'pack' must be a RaggedPack, not {type(pack).__name__}")
        if pack.C.dtype != torch.float64:
            raise TypeError(f"the packed costs must be torch.float64, not {pack.C.dtype}")
        k, max_rounds = _check_rounds(k, "k"), _check_rounds(max_rounds, "max_rounds")
        if not 1 <= k <= 256:
            raise ValueError(f"k must be in 1..256, not {k}")
        if max_rounds < 1:
            raise ValueError(f"max_rounds must be at least 1, not {max_rounds}")
        _check_pack_vector(pack, "seed", seed, optional=True)
        B, N, dev = len(pack.host_sizes), pack.N, pack.C.device
        x = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        y = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        v = torch.zeros((B, N), dtype=torch.float64, device=dev)
        ret, rounds, nnz, viol_last = [0] * B, [0] * B, [0] * B, [-1] * B

        csr, counts = self.prune_grow(pack, k, key=seed)
        added, _, gret = self.prune_counts(counts, B)
        csr.host_nnz = added
        ids = list(range(B))  # the instances behind `sub` and `csr`, in their order
        sub, r = pack, 0
        while True:
            keep = [q for q, b in enumerate(ids) if gret[q] == 0 and ret[b] == 0 and viol_last[b] != 0]
            for q, b in enumerate(ids):
                if gret[q] == 5 or (gret[q] != 0 and r > 0):  # (an admissible instance never gets there)
                    raise RuntimeError(f"lapjv_pruned_ragged: grow step {r} returned {gret[q]} for instance {b}")
                if gret[q] != 0:
                    ret[b] = gret[q]
            if r >= max_rounds:
                for q in keep:
                    ret[ids[q]] = 2
                keep = []
            if not keep:
                break
            # the live instances only: their offsets and sizes, the buffers as they are (N: lapmod_ragged's width)
            if len(keep) < len(ids) or sub.N != max(sub.host_sizes):
                idx = torch.tensor(keep, device=dev)
                hs = [sub.host_sizes[q] for q in keep]
                sub = RaggedPack(pack.C, sub.offsets[idx], sub.sizes[idx], None, None, pack.ld, max(hs), hs)
                csr = SparsePack(csr.cc, csr.kk, csr.ii, csr.nnz_offsets[idx], csr.row_offsets[idx], sub.sizes, hs,
                                 [csr.host_nnz[q] for q in keep])
                ids = [ids[q] for q in keep]
            sol = self.lapmod_ragged(csr, 3, want_stats=False)
            r += 1
            nxt, counts = self.prune_grow(sub, k, key=sol["v"], x=sol["x"], csr=csr, write=r < max_rounds)
            where = torch.tensor(ids, device=dev)
            x[where, :sub.N], y[where, :sub.N], v[where, :sub.N] = sol["x"], sol["y"], sol["v"]
            added, viol, gret, sret = self.prune_counts(counts, len(ids), sol["ret"])
            for q, b in enumerate(ids):
                if sret[q] != 0:
                    raise RuntimeError(f"lapjv_pruned_ragged: lapmod_ragged returned {sret[q]} for instance {b}")
                rounds[b], nnz[b], viol_last[b] = r, csr.host_nnz[q], viol[q]
            if nxt is not None:
                nxt.host_nnz = [nz + a for nz, a in zip(csr.host_nnz, added)]
                csr = nxt
        ret_d = torch.tensor(ret, dtype=torch.int32, device=dev)
        u = torch.empty((B, N), dtype=torch.float64, device=dev)
        cost = torch.empty((B,), dtype=torch.float64, device=dev)
        hip_call("lapwarm_prune_finish_ragged", "lapjv_pruned_ragged", dev, pack.C, pack.offsets, pack.sizes, pack.ld,
                 B, N, x, v, ret_d, u, cost)
        return {"x": x, "y": y, "u": u, "v": v, "cost": cost, "ret": ret_d,
                "rounds": torch.tensor(rounds, dtype=torch.int32, device=dev),
                "nnz": torch.tensor(nnz, dtype=torch.int64, device=dev),
                "viol_last": torch.tensor(viol_last, dtype=torch.int64, device=dev)}

    def _pruned_packed(self, pack, k, seed, max_rounds=32):
        """lapjv_pruned_ragged, and the dense route (lapjv_batch, one call per size) for the instances it leaves
        with ret 2 or 3: one dict per instance with x, y (n_b,) int32, cost, ret and fallback (bool) on the host
        side of the result, rounds and nnz."""
        out = self.lapjv_pruned_ragged(pack, k, seed, max_rounds)
        ret = out["ret"].tolist()
        x, y, cost = out["x"], out["y"], out["cost"].clone()
        redo = {}
        for b, n in enumerate(pack.host_sizes):
            if ret[b] in (2, 3):
                redo.setdefault(n, []).append(b)
        if redo:
            off = pack.offsets.tolist()
            stride = pack.ld or None
            for n, members in redo.items():
                ld = stride or n
                C = torch.stack([pack.C[off[b]:off[b] + (n - 1) * ld + n].as_strided((n, n), (ld, 1))
                                 for b in members]).contiguous()
                xd, yd, _, _ = self.lapjv_batch(C, want_stats=False)
                idx = torch.tensor(members, device=self.device)
                x[idx, :n], y[idx, :n] = xd, yd
                cost[idx] = torch.stack([C[q, torch.arange(n, device=self.device), xd[q].long()].sum()
                                         for q in range(len(members))])
        rounds, nnz = out["rounds"].tolist(), out["nnz"].tolist()
        return [{"x": x[b, :n], "y": y[b, :n], "cost": cost[b], "ret": ret[b], "fallback": ret[b] in (2, 3),
                 "rounds": rounds[b], "nnz": nnz[b]} for b, n in enumerate(pack.host_sizes)]

    @torch.inference_mode()
    def solve_pruned_many(self, costs, k: int = 16, use_model: bool = True, max_rounds: int = 32):
        """Optimal assignments of square fp64 matrices of different sizes through the pruned route: the seed of
        round 0 is predict_ragged's v_hat (the min-trick of the model's u_hat) with `use_model`, none without; an
        instance that is not certified within max_rounds or is not admissible (ret 2 or 3) is solved again by the
        dense lapjv_batch, so every instance comes back with an optimum.  One dict per instance, in input order:
        x, y (n_b,) int32, cost, ret (of the pruned solve), fallback, rounds, nnz."""
        if use_model:
            pack, _, v_hat = self._predict_ragged(costs)
        else:
            pack, v_hat = ragged_pack(costs, self.device), None
        return self._pruned_packed(pack, k, v_hat, max_rounds)

    def _extended_many_parts(self, costs, extend_cost=True, cost_limit=float("inf"), want_stats=True):
        """lapjv_extended_many before the results are cut up: a list of (indices, rows, cols, padded dict), one
        entry for the ragged call and one per lapjv_extended_batch call.  Argument errors come first."""
        mats = list(costs)
        limits = _limits_of(cost_limit, len(mats))
        extend_cost = int(bool(extend_cost))
        shapes = []
        for c in mats:
            if not isinstance(c, torch.Tensor):
                c = np.asarray(c)
            if c.ndim != 2:
                raise ValueError("2-dimensional array expected")
            shapes.append((int(c.shape[0]), int(c.shape[1])))
        sizes = []
        for (r, c), t in zip(shapes, limits):
            n = self.lib.lapwarm_lapjv_extended_n(r, c, extend_cost, t)
            if n == -4:
                raise ValueError(NONSQUARE)
            if n == -2:
                raise ValueError("lapjv_extended_many: non-empty cost matrices expected")
            sizes.append(_hip.check(n, "lapjv_extended_many"))
        # (a threads_hint picks another geometry than the plan the ragged launches are grouped by)
        ragged = [b for b, n in enumerate(sizes) if self.threads_hint == 0 and self.lapjv_ragged_eligible(n)]
        parts = []
        if ragged:
            pack = extended_pack([mats[b] for b in ragged], [limits[b] for b in ragged], self.device)
            parts.append((ragged, pack.host_rows, pack.host_cols,
                          self.lapjv_extended_ragged(pack, extend_cost, want_stats)))
        groups = {}
        taken = set(ragged)
        for b, (shape, t) in enumerate(zip(shapes, limits)):
            if b not in taken:
                groups.setdefault((shape, t), []).append(b)
        for ((r, c), t), members in groups.items():
            C = torch.stack([mats[b] if isinstance(mats[b], torch.Tensor)
                             else torch.from_numpy(np.ascontiguousarray(mats[b], dtype=np.float64))
                             for b in members]).to(self.device)
            parts.append((members, [r] * len(members), [c] * len(members),
                          self.lapjv_extended_batch(C, extend_cost, t, want_stats)))
        return len(mats), parts

    def lapjv_extended_many(self, costs, extend_cost: bool = True, cost_limit=float("inf"), want_stats: bool = True):
        """The reference's `lapjv(cost, extend_cost, cost_limit)` for instances of different shapes: `costs` is
        a sequence of 2-D fp64 arrays or CUDA tensors, `cost_limit` a scalar or one value per instance.  The
        instances lapjv_extended_ragged takes go through one call of it; the rest (extended size above the class
        of `lapjv_ragged_eligible`; every instance when this pipeline has a threads_hint) through
        lapjv_extended_batch, once per distinct shape and limit.  Returns one dict per instance, in input order:
        x (n_rows,), y (n_cols,) int32, opt, matched, ret, stats -- the rows of what lapjv_extended_batch returns
        for the instance alone."""
        count, parts = self._extended_many_parts(costs, extend_cost, cost_limit, want_stats)
        out = [None] * count
        for members, rows, cols, o in parts:
            for k, b in enumerate(members):
                out[b] = {"x": o["x"][k, :rows[k]], "y": o["y"][k, :cols[k]], "opt": o["opt"][k],
                          "matched": o["matched"][k], "ret": o["ret"][k],
                          "stats": o["stats"][k] if want_stats else None}
        return out

    def optimal_duals_batch(self, C: torch.Tensor):
        """Cold JV + the optimal duals it ends with: x (B,n) int32, u, v (B,n) fp64, ret.
        u_i = C[i, x_i] - v[x_i]; (u, v) is feasible and tight on the optimal assignment."""
        C = C.contiguous()
        B, n, _ = C.shape
        x = torch.empty((B, n), dtype=torch.int32, device=C.device)
        y = torch.empty((B, n), dtype=torch.int32, device=C.device)
        u = torch.empty((B, n), dtype=torch.float64, device=C.device)
        v = torch.empty((B, n), dtype=torch.float64, device=C.device)
        ret = torch.empty((B,), dtype=torch.int32, device=C.device)
        ws, nbytes = self._workspace(B, n, cold=True)
        hip_call("lapwarm_lapjv_duals_batched", "optimal_duals_batch", C.device, C, B, n, x, y, u, v, ret, None, ws,
                 nbytes, self.threads_hint)
        return x, u, v, ret

    def oracle_duals_batch(self, C: torch.Tensor, x: Optional[torch.Tensor] = None):
        """The reference's oracle duals (solvers/dual_computation.py:13-74) of a resident batch.
        x (B,n) int32 is the matching, row i -> column x[b][i]; None: the cold lapjv_batch matching.
        Returns x, u, v (B,n) fp64, ret (B,) int32 (0 ok, 1 negative cycle, 2 infeasible, 3 slackness,
        4 not a permutation, 5 non-finite C) and sweeps (B,4) int32: Jacobi sweeps, hop depth, rows
        read, replayed.  Synchronises the stream once per chunk of sweeps (not graph-capturable)."""
        C = C.contiguous()
        B, n, _ = C.shape
        if x is None:
            x, _, _, _ = self.lapjv_batch(C, want_stats=False)
        x = x.to(device=C.device, dtype=torch.int32).contiguous()
        rows = torch.arange(n, dtype=torch.int32, device=C.device).expand(B, n).contiguous()
        u = torch.empty((B, n), dtype=torch.float64, device=C.device)
        v = torch.empty((B, n), dtype=torch.float64, device=C.device)
        ret = torch.empty((B,), dtype=torch.int32, device=C.device)
        sweeps = torch.empty((B, 4), dtype=torch.int32, device=C.device)
        nbytes = int(self.lib.lapwarm_oracle_duals_workspace_bytes(B, n))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=C.device)
        hip_call("lapwarm_oracle_duals_batched", "oracle_duals_batch", C.device, C, B, n, rows, x, u, v, ret, sweeps,
                 ws, nbytes)
        return x, u, v, ret, sweeps

    def oracle_duals_ragged(self, pack: RaggedPack, x: torch.Tensor):
        """oracle_duals_batch of every instance of a ragged batch in one call (lapwarm_oracle_duals_ragged): one
        init and one shared chain of sweep launches, `pack.C` read where it is.  `pack` is a ragged_pack result;
        x (B, N) int32 or int64 on the device of the pack is the matching, row i -> column x[b][i] on the prefix
        of each instance (anything beyond it is ignored).  Returns u, v (B, N) fp64 (0 beyond the prefix; NaN
        on the prefix of an instance with ret 1, 4 or 5), ret (B,) int32 with the codes of oracle_duals_batch
        (and 6 for a size the device treats as empty) and sweeps (B, 4) int32; row b is, bit for bit, what
        oracle_duals_batch gives instance b alone.  Synchronises the stream once per chunk of sweeps (not
        graph-capturable).  Raises ValueError before any device work."""
        B, N, dev = len(pack.host_sizes), pack.N, pack.C.device
        if pack.C.dtype != torch.float64:
            raise ValueError(f"the packed costs must be float64, not {pack.C.dtype}")
        if not isinstance(x, torch.Tensor) or x.dtype not in (torch.int32, torch.int64):
            raise ValueError("x must be an int32 or int64 tensor")
        if tuple(x.shape) != (B, N):
            raise ValueError(f"x must be ({B}, {N}), not {tuple(x.shape)}")
        if x.device != dev:
            raise ValueError(f"x must be on {dev}, not {x.device}")
        cols = x.to(torch.int32).contiguous()
        rows = torch.arange(N, dtype=torch.int32, device=dev).expand(B, N).contiguous()
        u = torch.empty((B, N), dtype=torch.float64, device=dev)
        v = torch.empty((B, N), dtype=torch.float64, device=dev)
        ret = torch.empty((B,), dtype=torch.int32, device=dev)
        sweeps = torch.empty((B, 4), dtype=torch.int32, device=dev)
        ws, nbytes = self._cached_workspace(("oracle_ragged", B, N),
                                            lambda: self.lib.lapwarm_oracle_duals_ragged_workspace_bytes(B, N))
        host_sizes = (ct.c_int * B)(*pack.host_sizes)
        hip_call("lapwarm_oracle_duals_ragged", "oracle_duals_ragged", dev, pack.C, pack.offsets, pack.sizes,
                 host_sizes, pack.ld, B, N, rows, cols, u, v, ret, sweeps, ws, nbytes)
        return u, v, ret, sweeps

    def _matching_packed(self, pack, r=None):
        """x (B, N), -1 beyond n_b: the assignment the seeded solve of every instance ends at.  One
        seeded_ragged call where it takes every instance: x stays the padded tensor the solver wrote."""
        with torch.no_grad():
            pack, u, v = self._predict_packed(pack, r)
            if self.threads_hint == 0 and all(self.ragged_solve_eligible(n) for n in set(pack.host_sizes)):
                return self.seeded_ragged(pack, u, v, want_stats=False)[0]
            sol = self._solve_packed(pack, u, v, want_stats=False)
        return torch.nn.utils.rnn.pad_sequence([o["x"] for o in sol], batch_first=True, padding_value=-1)

    def _padded_matching(self, x, sizes, N, dev):
        """The caller's matchings as one (B, N) integer tensor on the device, -1 beyond n_b: a (B, N) tensor on
        the device is used as it is; a sequence of B vectors is padded on the device when every one is a tensor
        there, of one integer type, and otherwise on the host (one upload)."""
        B = len(sizes)
        if isinstance(x, torch.Tensor) and x.ndim == 2:
            if tuple(x.shape) != (B, N) or x.device != dev:
                raise ValueError(f"a padded x must be ({B}, {N}) on {dev}, not {tuple(x.shape)} on {x.device}")
            return x
        x = list(x)
        if len(x) != B:
            raise ValueError(f"{B} instances but {len(x)} matchings")
        on_device = all(isinstance(xb, torch.Tensor) and xb.device == dev and xb.dtype == x[0].dtype for xb in x)
        if not on_device:
            x = [np.asarray(xb.cpu() if isinstance(xb, torch.Tensor) else xb) for xb in x]
        for b, (xb, n) in enumerate(zip(x, sizes)):
            if tuple(xb.shape) != (n,):
                raise ValueError(f"matching {b} has shape {tuple(xb.shape)} for an instance of size {n}")
        if on_device:
            return torch.nn.utils.rnn.pad_sequence(x, batch_first=True, padding_value=-1)
        xh = np.full((B, N), -1, dtype=np.int32)
        for b, (xb, n) in enumerate(zip(x, sizes)):
            xh[b, :n] = xb
        return torch.from_numpy(xh).to(dev)

    def oracle_duals_many(self, costs, x=None):
        """The oracle duals of instances of different sizes: ragged_pack, then one oracle_duals_ragged call.
        costs: a sequence of square fp64 matrices, or one (B, n, n) float64 CUDA tensor of B instances of one
        size, which is read where it is.  x: one matching per instance (n_b values each, row i -> column), or
        one (B, N) integer tensor on the device, or None for the matching of solve_many.
        A seeded solve ends at an optimal assignment whatever the model predicts; where the optimum is unique
        that is the `lap.lapjv` matching and the duals have the reference's bits, and where costs tie another
        optimal matching may be chosen: the duals are then still optimal (feasible, tight on that matching) but
        need not be the ones the reference computes from its own matching.
        Returns a sequence with one (x, u, v, ret, sweeps) per instance, in input order, sliced to n_b: views of
        the padded results (its fields x, u, v, ret, sweeps), made when an entry is read."""
        if isinstance(costs, torch.Tensor) and costs.ndim == 3:
            pack = ragged_pack(costs, self.device, sizes=[costs.shape[1]] * costs.shape[0])
        else:
            pack = ragged_pack(costs, self.device)
        host_sizes, N = pack.host_sizes, pack.N
        xd = self._matching_packed(pack) if x is None else self._padded_matching(x, host_sizes, N, pack.C.device)
        u, v, ret, sweeps = self.oracle_duals_ragged(pack, xd)
        return RaggedDuals(xd, u, v, ret, sweeps, host_sizes)

    def training_batch(self, costs, dual_noise_std: float = 0.0, dual_noise_prob: float = 0.0, generator=None):
        """costs of different sizes -> a labelled DeviceBatch (gnn/collate.py) with no per-instance host work
        (where seeded_ragged takes every size; other sizes are solved per size, as in solve_many):
        one ragged_pack (the only upload of the costs), one ragged feature call (features, top-16, float32
        costs, mask), the matching of the seeded solve from this pipeline's model, and the ragged oracle duals
        of that matching as the float32 targets u, v (0 on padded rows).  Raises RuntimeError naming the first
        instance whose oracle duals fail, with its code.
        dual_noise_prob > 0 with dual_noise_std > 0 is the noisy-label recipe of the reference's data generator
        (data/generators.py:131-135) on the device: with that probability an instance's fp64 duals get N(0,
        dual_noise_std) noise and are projected back to feasibility in 75 rounds at most (noisy_duals_ragged, with
        `generator`); only u and v of the batch differ.  With the defaults nothing is added to the clean path."""
        dual_noise_std, dual_noise_prob = _check_noise_args(dual_noise_std, dual_noise_prob, generator,
                                                            ("dual_noise_std", "dual_noise_prob"))
        return self._training_batch_packed(ragged_pack(costs, self.device), dual_noise_std, dual_noise_prob, generator,
                                           "training_batch")

    def _training_batch_packed(self, pack, dual_noise_std, dual_noise_prob, generator, who):
        """training_batch of a batch that is packed already, its noise arguments checked."""
        from .collate import DeviceBatch
        r = row_features_packed(pack, return_topk=True, want_cost32=True)
        u, v = self._labels_packed(pack, r, dual_noise_std, dual_noise_prob, generator, who)
        return DeviceBatch(cost=r.cost32, u=u, v=v, row_feat=r.feat, topk=r.topk, mask=r.mask, sizes=r.sizes)

    def synthetic_training_batch(self, families, sizes, seeds, params=None, dual_noise_std: float = 0.0,
                                 dual_noise_prob: float = 0.0, generator=None):
        """training_batch of costs that are made on the device: gnn.synthetic.synthetic_pack(families, sizes, seeds,
        params=params) in place of ragged_pack, so no cost matrix exists on the host and none is uploaded.  Every
        field is bit for bit training_batch of those matrices."""
        from .synthetic import synthetic_pack
        dual_noise_std, dual_noise_prob = _check_noise_args(dual_noise_std, dual_noise_prob, generator,
                                                            ("dual_noise_std", "dual_noise_prob"))
        pack = synthetic_pack(families, sizes, seeds, self.device, params)
        return self._training_batch_packed(pack, dual_noise_std, dual_noise_prob, generator,
                                           "synthetic_training_batch")

    def _labels_packed(self, pack, r, dual_noise_std, dual_noise_prob, generator, who):
        """The label half of training_batch and dual_training_batch: the float32 targets u, v (B, N) of a packed
        batch, from the matching of the seeded solve and its ragged oracle duals, noisy where asked.  `r`: the row
        features of the pack (a OneGNN prediction reads them); `who` names the caller in the error."""
        x = self._matching_packed(pack, r)
        u, v, ret, _ = self.oracle_duals_ragged(pack, x)
        bad = torch.nonzero(ret).reshape(-1).tolist()
        if bad:
            raise RuntimeError(f"{who}: oracle duals of instance {bad[0]} (n = {pack.host_sizes[bad[0]]}) "
                               f"failed with code {int(ret[bad[0]])}")
        if dual_noise_prob > 0.0 and dual_noise_std > 0.0:
            u, v, _ = self.noisy_duals_ragged(pack, u, v, dual_noise_std, generator=generator, prob=dual_noise_prob)
        return u.to(torch.float32), v.to(torch.float32)

    def dual_training_batch(self, costs, dual_noise_std: float = 0.0, dual_noise_prob: float = 0.0, generator=None):
        """costs of different sizes -> a labelled DualDeviceBatch (gnn/collate.py), the reference's `collate`
        (gnn/train.py:64-95) with the labels made on the device and no per-instance host work: one ragged_pack (the
        only upload of the costs), the ragged graph features (edge, row and column features, mask), the float32
        costs, then the label half of training_batch: the matching of the seeded solve from this pipeline's model,
        the ragged oracle duals of that matching as the float32 targets u, v (0 on padded rows) and, with
        dual_noise_prob > 0 and dual_noise_std > 0, its noisy-label recipe with `generator`.  u and v are bit for
        bit those of training_batch for the same costs.  The graph features limit every size to n <= 4096: a
        larger one raises the ValueError of graph_features_packed.  Raises RuntimeError naming the first instance
        whose oracle duals fail, with its code.  The method of a DualWarmStartPipeline: like the prediction, it goes
        by the model's type, and a pipeline around another model raises TypeError."""
        dual_noise_std, dual_noise_prob = self._check_dual_training_args(dual_noise_std, dual_noise_prob, generator,
                                                                         "dual_training_batch")
        return self._dual_training_batch_packed(ragged_pack(costs, self.device), dual_noise_std, dual_noise_prob,
                                                generator, "dual_training_batch")

    def _check_dual_training_args(self, dual_noise_std, dual_noise_prob, generator, who):
        dual_noise_std, dual_noise_prob = _check_noise_args(dual_noise_std, dual_noise_prob, generator,
                                                            ("dual_noise_std", "dual_noise_prob"))
        if not isinstance(self.model, DualGNN):
            raise TypeError(f"{who} needs a pipeline around a DualGNN (DualWarmStartPipeline), not "
                            f"{type(self.model).__name__}")
        return dual_noise_std, dual_noise_prob

    def synthetic_dual_training_batch(self, families, sizes, seeds, params=None, dual_noise_std: float = 0.0,
                                      dual_noise_prob: float = 0.0, generator=None):
        """dual_training_batch of costs that are made on the device (gnn.synthetic.synthetic_pack in place of
        ragged_pack): bit for bit dual_training_batch of those matrices, with no matrix on the host."""
        from .synthetic import synthetic_pack
        dual_noise_std, dual_noise_prob = self._check_dual_training_args(dual_noise_std, dual_noise_prob, generator,
                                                                         "synthetic_dual_training_batch")
        pack = synthetic_pack(families, sizes, seeds, self.device, params)
        return self._dual_training_batch_packed(pack, dual_noise_std, dual_noise_prob, generator,
                                                "synthetic_dual_training_batch")

    def _dual_training_batch_packed(self, pack, dual_noise_std, dual_noise_prob, generator, who):
        """dual_training_batch of a batch that is packed already, its other arguments checked."""
        from .collate import DualDeviceBatch
        f = graph_features_packed(pack)
        r = row_features_packed(pack, return_topk=False, want_cost32=True)  # the float32 cast, padded with 0
        u, v = self._labels_packed(pack, r, dual_noise_std, dual_noise_prob, generator, who)
        return DualDeviceBatch(cost=r.cost32, u=u, v=v, row_feat=f.row, col_feat=f.col, edge_feat=f.edge, mask=f.mask,
                               sizes=f.sizes)

    # ---- dual utilities of a ragged batch (csrc/ragged_batch.hip): solvers/advanced_dual.py:14-63 and the
    # classical seeds of solvers/seed_baselines.py for every instance of a pack in one call each
    def _check_duals_args(self, pack, u, v):
        """Argument errors, raised before any device work: types and dtypes, then shapes, then devices."""
        if not isinstance(pack, RaggedPack):
            raise TypeError(f"Argument 'pack' must be a RaggedPack, not {type(pack).__name__}")
        if pack.C.dtype != torch.float64:
            raise TypeError(f"the packed costs must be torch.float64, not {pack.C.dtype}")
        _check_pack_vector(pack, "u", u)
        _check_pack_vector(pack, "v", v)
        return len(pack.host_sizes), pack.N, pack.C.device

    def _duals_workspace(self, B, N):
        return self._cached_workspace(("ragged_duals", B, N),
                                      lambda: self.lib.lapwarm_ragged_duals_workspace_bytes(B, N))

    def _project_ragged(self, pack, sizes, u, v, max_rounds, tol):
        """lapwarm_project_feasible_ragged on u, v in place; `sizes` (B,) int32 on the device is pack.sizes, or a
        copy with 0 for the instances to leave out."""
        B, N, dev = len(pack.host_sizes), pack.N, pack.C.device
        gmin = torch.empty((B,), dtype=torch.float64, device=dev)
        rounds = torch.empty((B,), dtype=torch.int32, device=dev)
        ret = torch.empty((B,), dtype=torch.int32, device=dev)
        ws, nbytes = self._duals_workspace(B, N)
        hip_call("lapwarm_project_feasible_ragged", "project_feasible_ragged", dev, pack.C, pack.offsets, sizes,
                 pack.ld, B, N, u, v, int(max_rounds), float(tol), gmin, rounds, ret, ws, nbytes)
        return u, v, gmin, rounds, ret

    def project_feasible_ragged(self, pack: RaggedPack, u: torch.Tensor, v: torch.Tensor, max_rounds: int = 50,
                                tol: float = 1e-12):
        """project_feasible (solvers/advanced_dual.py:14-36) of every instance of a ragged batch in one call.
        u, v (B, N) fp64 on the device of the pack, read on each prefix and left as they are.  Returns new u, v
        (B, N) fp64 (0 beyond n_b), gmin (B,) fp64 the last min((C - u) - v), rounds (B,) int32 the rounds each
        instance ran (it stops on its own, on the device) and ret (B,) int32 (0; 2 for a size the device treats
        as empty).  Row b is, bit for bit, what solvers.project_feasible gives instance b alone.  Synchronises
        the stream once per chunk of rounds after the first round (not graph-capturable when max_rounds > 1)."""
        self._check_duals_args(pack, u, v)
        max_rounds, tol = _check_rounds(max_rounds, "max_rounds"), _check_real(tol, "tol")
        return self._project_ragged(pack, pack.sizes, u.clone(), v.clone(), max_rounds, tol)

    def reduce_costs_ragged(self, pack: RaggedPack, u: torch.Tensor, v: torch.Tensor, shift_nonneg: bool = True,
                            want_matrix: bool = True):
        """reduce_costs (solvers/advanced_dual.py:39-53) of every instance of a ragged batch: returns (out, gmin,
        ret).  out, a tensor like pack.C (the same offsets and row stride; 0 in the padding of a padded layout),
        holds (C - u) - v of every instance, minus its minimum where shift_nonneg and that is negative; None
        without want_matrix.  gmin (B,) fp64 is the unshifted minimum, ret (B,) int32 0 or 2.  Bit for bit
        solvers.reduce_costs per instance.  Kernels on the current stream only."""
        B, N, dev = self._check_duals_args(pack, u, v)
        out = None
        if want_matrix:
            out = torch.empty_like(pack.C) if pack.ld == 0 else torch.zeros_like(pack.C)
        gmin = torch.empty((B,), dtype=torch.float64, device=dev)
        ret = torch.empty((B,), dtype=torch.int32, device=dev)
        ws, nbytes = self._duals_workspace(B, N)
        hip_call("lapwarm_reduce_costs_ragged", "reduce_costs_ragged", dev, pack.C, pack.offsets, pack.sizes, pack.ld,
                 B, N, u, v, int(bool(shift_nonneg)), out, gmin, ret, ws, nbytes)
        return out, gmin, ret

    def dual_feasible_ragged(self, pack: RaggedPack, u: torch.Tensor, v: torch.Tensor, tol: float = 1e-8):
        """check_dual_feasible (solvers/advanced_dual.py:56-63) of every instance: a (B,) bool tensor on the
        device, False where the reference raises (min((C - u) - v) < -tol; NaN passes, as it does there).  It
        does not raise and nothing is read back."""
        self._check_duals_args(pack, u, v)
        tol = _check_real(tol, "tol")
        _, gmin, _ = self.reduce_costs_ragged(pack, u, v, shift_nonneg=False, want_matrix=False)
        return ~(gmin < -tol)

    def seed_row_col_minima_ragged(self, pack: RaggedPack, project_rounds: int = 50):
        """seed_row_col_minima (solvers/seed_baselines.py:18-37) of every instance: the row minima, the ragged
        min-trick of them, then the ragged projection.  Returns what project_feasible_ragged returns."""
        if not isinstance(pack, RaggedPack):
            raise TypeError(f"Argument 'pack' must be a RaggedPack, not {type(pack).__name__}")
        project_rounds = _check_rounds(project_rounds, "project_rounds")
        u = row_min_ragged(pack)
        v = min_trick_ragged(pack, u)
        return self._project_ragged(pack, pack.sizes, u, v, project_rounds, 1e-12)

    def noisy_duals_ragged(self, pack: RaggedPack, u: torch.Tensor, v: torch.Tensor, noise_std: float,
                           project_rounds: int = 75, generator=None, prob: float = 1.0):
        """Perturbed and re-projected duals of a ragged batch (solvers/seed_baselines.py:91-110; with `prob` the
        recipe of data/generators.py:131-135), on the device.  One Bernoulli draw per instance with `prob`
        decides whether it is perturbed; a perturbed instance gets u + N(0, noise_std), v + N(0, noise_std)
        (fp64 torch.randn on the device, from `generator`, used on its prefix) and then the ragged projection,
        in which the other instances take no part: they keep u, v bit for bit.  The draws are (B, N) normals
        for u, (B, N) for v, then (B,) uniforms, in that order, whatever `prob` is.  Returns u, v (B, N) fp64
        and the (B,) bool tensor of perturbed instances; the inputs are left as they are."""
        B, N, dev = self._check_duals_args(pack, u, v)
        noise_std, prob = _check_noise_args(noise_std, prob, generator, ("noise_std", "prob"))
        project_rounds = _check_rounds(project_rounds, "project_rounds")
        if generator is not None and generator.device.type != dev.type:
            raise ValueError(f"generator must be on {dev} like the packed costs, not {generator.device}")
        nu = torch.randn((B, N), dtype=torch.float64, device=dev, generator=generator)
        nv = torch.randn((B, N), dtype=torch.float64, device=dev, generator=generator)
        hit = torch.rand((B,), dtype=torch.float64, device=dev, generator=generator) < prob
        prefix = torch.arange(N, device=dev).unsqueeze(0) < pack.sizes.unsqueeze(1)
        take = prefix & hit.unsqueeze(1)
        un = torch.where(take, u + noise_std * nu, u).contiguous()
        vn = torch.where(take, v + noise_std * nv, v).contiguous()
        # an instance that is not perturbed is given size 0: the projection treats it as empty and gives it no work
        sizes = torch.where(hit, pack.sizes, torch.zeros_like(pack.sizes)).contiguous()
        self._project_ragged(pack, sizes, un, vn, project_rounds, 1e-12)
        keep = ~hit.unsqueeze(1)
        return torch.where(keep, u, un), torch.where(keep, v, vn), hit

    @torch.inference_mode()
    def solve_batch(self, C: torch.Tensor, eps: float = 1e-12, want_stats: bool = True) -> dict:
        """The whole hot path for a resident batch."""
        u, v = self.predict_batch(C)
        x, y, ret, stats = self.seeded_batch(C, u, v, eps, want_stats)
        return {"x": x, "y": y, "ret": ret, "stats": stats, "u": u, "v": v}

    def _predict_ragged(self, costs):
        return self._predict_packed(ragged_pack(costs, self.device))

    def _predict_packed(self, pack, r=None):
        """(pack, u_hat, v_hat) of a packed batch; `r`: its row features, where the caller has them already."""
        if isinstance(self.model, DualGNN):
            return _predict_packed_dual(self.model, pack)
        if r is None:
            r = row_features_packed(pack)
        u = self.model(r.feat, mask=r.mask, topk_values=r.topk)["u"].to(torch.float64)
        u = _centre_per_instance(u, pack.sizes, r.mask)
        return pack, u, min_trick_ragged(pack, u)

    @torch.inference_mode()
    def predict_ragged(self, costs):
        """costs: square fp64 matrices of different sizes (NumPy, or CUDA tensors) -> a list of (u_hat, v_hat),
        fp64 device tensors of length n_b, what predict_batch gives each instance alone: ragged features and
        top-16, one masked OneGNN forward over the padded batch, then the fp64 min-trick of u_hat per instance
        (lapwarm_colmin_ragged).  With a DualGNN as the model: ragged graph features and one forward with the
        sizes (_predict_packed_dual); u_hat then agrees with predict_batch within float32 rounding, not bit for
        bit, because the torch GEMMs of the forward see another shape."""
        pack, u, v = self._predict_ragged(costs)
        return [(u[b, :n], v[b, :n]) for b, n in enumerate(pack.host_sizes)]

    def seeded_ragged(self, pack: RaggedPack, u: torch.Tensor, v: torch.Tensor, eps: float = 1e-12,
                      want_stats: bool = True):
        """lapjv_seeded of every instance of a ragged batch in one call (lapwarm_seeded_ragged): one solver
        launch per kernel configuration, not per size, and `pack.C` is read where it is.  `pack` is a
        ragged_pack result, u, v (B, N) fp64 (read on each instance's prefix).  Returns x, y (B, N) int64 with -1
        beyond n_b, ret (B,) int32, stats (B, 32) int64 or None; row b is what seeded_batch gives instance b
        alone with threads_hint 0: the launches follow the automatic plan, and this pipeline's threads_hint does not
        apply here (solve_many keeps the per-size path when one is set).  Every size must be in the class
        `ragged_solve_eligible` describes."""
        B, N, dev = len(pack.host_sizes), pack.N, pack.C.device
        for name, t in (("u", u), ("v", v)):
            if t.dtype != torch.float64 or tuple(t.shape) != (B, N) or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{name} must be a contiguous float64 ({B}, {N}) tensor on {dev}")
        x, y, ret, stats = _solve_outputs(B, N, torch.int64, dev, want_stats, ragged=True)
        ws, nbytes = self._cached_workspace(("seeded_ragged", B, N),
                                            lambda: self.lib.lapwarm_seeded_ragged_workspace_bytes(B, N))
        host_sizes = (ct.c_int * B)(*pack.host_sizes)
        hip_call("lapwarm_seeded_ragged", "seeded_ragged", dev, pack.C, pack.offsets, pack.sizes, host_sizes, pack.ld,
                 B, N, u, v, float(eps), x, y, ret, stats, ws, nbytes)
        return x, y, ret, stats

    def ragged_solve_eligible(self, n: int) -> bool:
        """Does seeded_ragged take an instance of this size?  Those whose own solve plan is one launch with
        all solver state in LDS and no helper workgroup: every n < 1024 and the odd n up to 3631 with
        the default settings (the library decides, from the plan)."""
        known = self._ragged_ok
        if n not in known:
            one = (ct.c_int * 1)(int(n))
            known[n] = self.lib.lapwarm_seeded_ragged_groups(one, 1, (ct.c_int * 1)()) == 1
        return known[n]

    @torch.inference_mode()
    def solve_many(self, costs, eps: float = 1e-12, want_stats: bool = True):
        """The whole hot path for instances of different sizes: predict_ragged, then seeded_ragged for every
        instance it takes (one solver launch per kernel configuration, the packed costs read in place) and
        seeded_batch once per size for the rest (helper or global-state sizes, the cooperative chain; every
        instance when this pipeline has a threads_hint).
        Returns one dict per instance, in input order: x, y (n_b,) int64, ret, stats, u, v -- the rows of what
        solve_batch returns for a batch of that size."""
        return self._solve_packed(*self._predict_ragged(costs), eps, want_stats)

    def _solve_packed(self, pack, u, v, eps=1e-12, want_stats=True):
        """solve_many behind the prediction: the seeded solves of a packed batch from u, v (B, N) fp64."""
        sizes = pack.host_sizes
        out = [None] * len(sizes)
        # (a threads_hint picks another geometry than the plan the ragged launches are grouped by: per-size path)
        ragged = [b for b, n in enumerate(sizes) if self.threads_hint == 0 and self.ragged_solve_eligible(n)]
        if ragged:
            sub, us, vs = pack, u, v
            if len(ragged) < len(sizes):  # the eligible instances only: their offsets and sizes, C as it is
                idx = torch.tensor(ragged, device=self.device)
                sub = RaggedPack(pack.C, pack.offsets[idx], pack.sizes[idx], None, None, pack.ld, pack.N,
                                 [sizes[b] for b in ragged])
                us, vs = u[idx], v[idx]
            x, y, ret, stats = self.seeded_ragged(sub, us, vs, eps, want_stats)
            for k, b in enumerate(ragged):
                n = sizes[b]
                out[b] = {"x": x[k, :n], "y": y[k, :n], "ret": ret[k], "stats": stats[k] if want_stats else None,
                          "u": us[k, :n], "v": vs[k, :n]}
        groups = {}
        for b, n in enumerate(sizes):
            if out[b] is None:
                groups.setdefault(n, []).append(b)
        off = pack.offsets.tolist() if groups else None
        for n, members in groups.items():
            C = torch.stack([pack.C[off[b]:off[b] + n * n].view(n, n) for b in members])
            idx = torch.tensor(members, device=self.device)
            ug, vg = u[idx, :n], v[idx, :n]
            x, y, ret, stats = self.seeded_batch(C, ug, vg, eps, want_stats)
            for k, b in enumerate(members):
                out[b] = {"x": x[k], "y": y[k], "ret": ret[k], "stats": stats[k] if want_stats else None,
                          "u": ug[k], "v": vg[k]}
        return out

    # ---- two-stream software pipeline: the dense sweeps + OneGNN of batch k+1 run beside the
    # per-instance solver of batch k.  The solver occupies one CU per instance (32 of the 256 at
    # K3), the sweeps want the rest; results are identical to solve_batch().
    def _streams(self):
        if not hasattr(self, "_s_pred"):
            self._s_pred = torch.cuda.Stream(self.device)
            self._s_solve = torch.cuda.Stream(self.device)
            self._pending = None
        return self._s_pred, self._s_solve

    @torch.inference_mode()
    def pipeline_submit(self, C: torch.Tensor, predict=None):
        """Enqueue features + OneGNN + min-trick for `C` on the prediction stream.  `predict(C) -> (u, v)`
        replaces the model-based prediction (K2: given duals, features + min-trick only)."""
        s_pred, _ = self._streams()
        s_pred.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s_pred):
            u, v = (predict or self.predict_batch)(C)
            ev = torch.cuda.Event()
            ev.record(s_pred)
        self._pending = (C, u, v, ev)
        self._predict = predict

    @torch.inference_mode()
    def pipeline_step(self, C_next: Optional[torch.Tensor] = None, eps: float = 1e-12,
                      want_stats: bool = True) -> dict:
        """Solve the batch submitted last (its duals are ready or being computed on the prediction
        stream), and submit `C_next` so that its dense stages overlap this solve.  The returned
        tensors are produced on the solver stream: synchronise (or wait on out["done"]) before
        reading them."""
        if self._pending is None:
            raise RuntimeError("pipeline_submit() first")
        _, s_solve = self._streams()
        C, u, v, ev = self._pending
        self._pending = None
        s_solve.wait_event(ev)
        with torch.cuda.stream(s_solve):
            x, y, ret, stats = self.seeded_batch(C, u, v, eps, want_stats)
            done = torch.cuda.Event()
            done.record(s_solve)
        for t in (C, u, v):
            t.record_stream(s_solve)
        # the results were allocated on the solver stream's pool and are consumed on the caller's
        for t in (x, y, ret) + ((stats,) if stats is not None else ()):
            t.record_stream(torch.cuda.current_stream(self.device))
        if C_next is not None:
            self.pipeline_submit(C_next, getattr(self, "_predict", None))
        return {"x": x, "y": y, "ret": ret, "stats": stats, "u": u, "v": v, "done": done}

    def pipeline_drain(self):
        s_pred, s_solve = self._streams()
        s_pred.synchronize()
        s_solve.synchronize()
        self._pending = None


def _centre_per_instance(u, sizes, mask):
    """u (B, N) fp64, 0 on padded rows, centred over the padded width -> centred over each instance's own rows.
    Both models centre u over all N slots (masked rows included, as the reference's forwards do), which shifts every
    instance shorter than the batch maximum; centred over its own rows an instance gets what the model gives it
    alone."""
    count = sizes.to(torch.float64).unsqueeze(1)
    return ((u - u.sum(dim=1, keepdim=True) / count) * mask).contiguous()


def _predict_packed_dual(model, pack):
    """WarmStartPipeline._predict_packed for a DualGNN: the ragged graph features, one forward over the padded batch
    with the sizes (the fused kernels skip the padding), u centred per instance in fp64, then the ragged fp64
    min-trick; the model's v_hint is not used."""
    f = graph_features_packed(pack)
    u = model(f.edge, f.row, f.col, sizes=f.sizes)["u"].to(torch.float64)
    u = _centre_per_instance(u, pack.sizes, f.mask)
    return pack, u, min_trick_ragged(pack, u)


class DualWarmStartPipeline(WarmStartPipeline):
    """The warm-start pipeline with DualGNN as its model: graph features -> DualGNN u -> v = min(C - u) ->
    lapjv_seeded.  Only the prediction differs; solve_batch, the pipeline_* methods and every solver entry are
    inherited.  So are predict_ragged and solve_many: their prediction (WarmStartPipeline._predict_packed) goes by
    the model's type, and for a DualGNN it is the ragged graph features and one forward with `sizes`."""

    @torch.inference_mode()
    def predict_batch(self, C: torch.Tensor):
        """C (B,n,n) f64 CUDA -> u (B,n) f32, v (B,n) f64 by the fp64 min-trick, as the harness does
        (scripts/gnn_benchmark.py:262); the model's v_hint is not used."""
        edge, row, col = graph_features_device(C)
        u = self.model(edge, row, col)["u"]
        v = min_trick_device(C, u)
        return u, v


_shared = {}


def shared_pipeline(device="cuda:0") -> WarmStartPipeline:
    """One WarmStartPipeline per process and device for callers that need its entries and workspaces but not a
    trained model (the NumPy-facing helpers of `solvers`): built on first use, with an untrained OneGNN."""
    key = str(torch.device(device))
    if key not in _shared:
        _shared[key] = WarmStartPipeline(OneGNN(ROW_FEATURE_DIM), device)
    return _shared[key]


class GNNPredictor:
    """`GNNPredictor(model_path).predict(C) -> (u, v)`, float64 NumPy, as the reference's
    harness expects (scripts/gnn_benchmark.py:213-289).  A ready OneGNN may be passed instead of
    a checkpoint path (`GNNPredictor(model=...)`)."""

    def __init__(self, model_path: Optional[str] = None, device: Optional[str] = None,
                 model: Optional[OneGNN] = None):
        self.model_path = model_path
        self.device = device or "cuda:0"
        if "cuda" not in str(self.device):
            raise RuntimeError("this GNNPredictor runs on the MI355X only; the CPU forward lives in the "
                               "reference / the test oracle")
        self.use_cuda = True
        self.row_only = True
        self.model_info = {}
        if model is None:
            if model_path is None:
                raise ValueError("model_path or model required")
            model, self.model_info = load_checkpoint(Path(model_path), self.device)
        self.model = model.to(self.device).eval()
        self._pipe = WarmStartPipeline(self.model, self.device)

    def predict(self, C: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        C = np.asarray(C, dtype=np.float64)
        Cd = torch.from_numpy(np.ascontiguousarray(C)).to(self.device).unsqueeze(0)
        u, v = self._pipe.predict_batch(Cd)
        torch.cuda.synchronize()
        return u[0].cpu().numpy().astype(np.float64), v[0].cpu().numpy().astype(np.float64)


class DualGNNPredictor:
    """`DualGNNPredictor(model_path).predict(C) -> (u, v)`, float64 NumPy, like GNNPredictor, for DualGNN
    checkpoints (load_dual_checkpoint).  A ready DualGNN may be passed instead (`DualGNNPredictor(model=...)`)."""

    def __init__(self, model_path: Optional[str] = None, device: Optional[str] = None,
                 model: Optional[DualGNN] = None):
        self.model_path = model_path
        self.device = device or "cuda:0"
        if "cuda" not in str(self.device):
            raise RuntimeError("this DualGNNPredictor runs on the MI355X only")
        self.use_cuda = True
        self.row_only = False
        self.model_info = {}
        if model is None:
            if model_path is None:
                raise ValueError("model_path or model required")
            model, self.model_info = load_dual_checkpoint(Path(model_path), self.device)
        self.model = model.to(self.device).eval()
        self._pipe = DualWarmStartPipeline(self.model, self.device)

    def predict(self, C: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        C = np.asarray(C, dtype=np.float64)
        Cd = torch.from_numpy(np.ascontiguousarray(C)).to(self.device).unsqueeze(0)
        u, v = self._pipe.predict_batch(Cd)
        torch.cuda.synchronize()
        return u[0].cpu().numpy().astype(np.float64), v[0].cpu().numpy().astype(np.float64)
