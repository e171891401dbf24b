"""The keep rule of DualGNN's fused dropout (csrc/dual_dropout.hpp) restated in NumPy, the masks of the two logical
tensors, the dropped formulations in torch, and the seeds that the GPU tests use -- TEST INFRASTRUCTURE, no GPU needed.

Philox4x32-10: key (lo32(seed), hi32(seed)), counter (lo32(e >> 2), hi32(e >> 2), stream, 0), the word of element e is
output e & 3; e is kept iff word >= floor(p 2^32); a kept value is multiplied by float32(1 / (1 - p))."""
import math

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM_EDGE, STREAM_ATTN = 0, 1
EDGE_HIDDEN = 128
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox_round(c, k):
    """One round: (c0, c1, c2, c3), (k0, k1) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).
    Every word is a uint64 array that holds a value below 2^32."""
    p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
    return ((p1 >> _32) ^ c[1] ^ k[0], p1 & _LO, (p0 >> _32) ^ c[3] ^ k[1], p0 & _LO)


def philox4x32_10(counter, key):
    """counter: four words, key: two words (ints or arrays) -> the four output words as uint64 arrays."""
    shape = np.broadcast(*[np.asarray(w) for w in (*counter, *key)]).shape
    c = tuple(np.broadcast_to(np.asarray(w, dtype=np.uint64), shape) for w in counter)
    k = tuple(np.broadcast_to(np.asarray(w, dtype=np.uint64), shape) for w in key)
    for r in range(10):
        if r:
            k = ((k[0] + np.uint64(W0)) & _LO, (k[1] + np.uint64(W1)) & _LO)
        c = philox_round(c, k)
    return c


def threshold(p):
    return int(math.floor(float(p) * 4294967296.0))


def scale(p):
    return np.float32(1.0 / (1.0 - float(p)))


def _words_of_groups(seed, stream, groups):
    seed = int(seed) & (2**64 - 1)
    groups = np.asarray(groups, dtype=np.uint64)
    out = philox4x32_10((groups & _LO, groups >> _32, stream, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=-1)  # (..., 4)


def keep_range(seed, stream, first, count, p):
    """bool (count,): the keep flags of the elements first .. first + count - 1 (one Philox call per four)."""
    first, count = int(first), int(count)
    g0, g1 = first >> 2, (first + count - 1) >> 2
    words = _words_of_groups(seed, stream, np.arange(g0, g1 + 1, dtype=np.uint64)).reshape(-1)
    at = first - 4 * g0
    return words[at:at + count] >= np.uint64(threshold(p))


def keep_elements(seed, stream, elements, p):
    """bool, the shape of `elements` (any 64-bit indices): one Philox call per element."""
    e = np.asarray(elements, dtype=np.uint64)
    words = _words_of_groups(seed, stream, e >> np.uint64(2))
    word = np.take_along_axis(words, (e & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]
    return word >= np.uint64(threshold(p))


def edge_mask(seed, p, B, N):
    """float32 (B, N, N, 128): scale or 0, element ((b N + i) N + j) 128 + unit of stream 0."""
    keep = keep_range(seed, STREAM_EDGE, 0, B * N * N * EDGE_HIDDEN, p).reshape(B, N, N, EDGE_HIDDEN)
    return torch.from_numpy(np.where(keep, scale(p), np.float32(0.0)).astype(np.float32))


def attn_mask(seed, p, B, H, N):
    """float32 (B, 2, H, N, N) as [query][key] in both directions: element (((b 2 + dir) H + h) N + q) N + k of
    stream 1."""
    keep = keep_range(seed, STREAM_ATTN, 0, B * 2 * H * N * N, p).reshape(B, 2, H, N, N)
    return torch.from_numpy(np.where(keep, scale(p), np.float32(0.0)).astype(np.float32))


def layer_seeds(generator, layers):
    """The seeds DualGNN draws from `generator` for `layers` layers, in forward order."""
    return [int(torch.randint(0, 2**63 - 1, (1,), dtype=torch.int64, generator=generator)) for _ in range(layers)]


# ---- the dropped formulations, in the dtype of the arguments ---------------------------------------------------

def edge_scores_torch(edge, W1_, b1, W2_, b2, G, mask0):
    """dual_gnn_common.edge_scores_torch with h1 multiplied by mask0 (B, N, N, 128)."""
    gelu = torch.nn.functional.gelu
    h1 = gelu(edge @ W1_.T + b1) * mask0.to(edge.dtype)
    h2 = gelu(h1 @ W2_.T + b2)
    s = torch.einsum("bijk,ok->boij", h2, G)
    B, _, N, _ = s.shape
    return s.reshape(B, 2, G.shape[0] // 2, N, N)


def attention_torch(scores, a_row, c_row, a_col, c_col, kbias, mask, row_val, col_val, mask1):
    """dual_gnn_common.attention_torch with the softmax weights multiplied by mask1 (B, 2, H, query, key)."""
    B, _, H, N, _ = scores.shape
    D = row_val.shape[-1] // H
    keep = mask if mask is not None else torch.ones((B, N), dtype=torch.bool)
    pair = keep[:, None, :, None] & keep[:, None, None, :]

    def one(s, a, c, k, val, m):  # s, m (B, H, query, key)
        s = torch.nn.functional.leaky_relu(a[..., :, None] + c[..., None, :] + s + k[None, :, None, None], 0.2)
        s = s.masked_fill(~pair, float("-inf"))
        w = torch.softmax(s, dim=-1)
        w = torch.where(torch.isfinite(w), w, torch.zeros_like(w)) * m.to(s.dtype)
        return torch.einsum("bhqk,bkhd->bqhd", w, val.reshape(B, N, H, D)).reshape(B, N, H * D)

    row_msg = one(scores[:, 0], a_row, c_row, kbias[:H], col_val, mask1[:, 0])
    col_msg = one(scores[:, 1].transpose(-1, -2), a_col, c_col, kbias[H:], row_val, mask1[:, 1])
    return row_msg, col_msg


class MaskMul(torch.nn.Module):
    """Stands in for an nn.Dropout of the plain path: call i multiplies by masks[i % len(masks)]."""

    def __init__(self, masks):
        super().__init__()
        self.masks, self.calls = list(masks), 0

    def forward(self, x):
        m = self.masks[self.calls % len(self.masks)]
        self.calls += 1
        return x * m.to(x.dtype)


def install_masks(model, seeds, p, B, N):
    """In a plain-path DualGNN: every other nn.Dropout gets p = 0, edge_mlp[2] becomes the multiplication with the
    stream-0 mask of the layer's seed and layer.dropout that with the stream-1 masks (row direction, then column
    direction, the order of DualLayer._messages_plain)."""
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    for layer, seed in zip(model.layers, seeds):
        layer.edge_mlp[2] = MaskMul([edge_mask(seed, p, B, N)])
        m1 = attn_mask(seed, p, B, layer.heads, N)
        layer.dropout = MaskMul([m1[:, 0], m1[:, 1]])


# ---- the fixed seeds of tests/test_gpu_dual_dropout.py ----------------------------------------------------------

P = 0.1
SEED_KEEP = 0x8000_0000_0000_0000 | 0x1234_5678_9ABC   # bit 63 set
KEEP_FIRST, KEEP_COUNT = 2**34 + 3, 4099
SEED_EDGE, SEED_ATTN, SEED_EDGE_BWD = 1234, 4321, 97
MODEL_GENERATOR_SEED, MODEL_LAYERS = 7, 2
EDGE_SHAPES = ((2, 17), (3, 17))                       # (B, N) of the edge forward
ATTN_SHAPES = ((2, 65, 4, 8), (2, 33, 2, 160))         # (B, N, H, D)
EDGE_BWD_SHAPES = ((1, 17), (2, 130), (3, 130))
MODEL_SHAPES = ((3, 40, 4), (3, 17, 4))                # (B, N, H): h32_H4_L2@pad, and the sizes (5, 17, 12)


def gpu_masks():
    """[(label, seed, stream, first, count, p)]: every mask the GPU tests draw."""
    out = [(f"keep p={p} stream={s}", SEED_KEEP, s, KEEP_FIRST, KEEP_COUNT, p) for p in (0.1, 0.5) for s in (0, 1)]
    out += [(f"edge forward {B}x{N}", SEED_EDGE, 0, 0, B * N * N * EDGE_HIDDEN, P) for B, N in EDGE_SHAPES]
    out += [(f"attention {B}x{N} H={H}", SEED_ATTN, 1, 0, B * 2 * H * N * N, P) for B, N, H, _ in ATTN_SHAPES]
    out += [(f"edge backward {B}x{N}", SEED_EDGE_BWD, 0, 0, B * N * N * EDGE_HIDDEN, P) for B, N in EDGE_BWD_SHAPES]
    for k, seed in enumerate(layer_seeds(torch.Generator().manual_seed(MODEL_GENERATOR_SEED), MODEL_LAYERS)):
        for B, N, H in MODEL_SHAPES:
            out.append((f"model {B}x{N} layer {k} edge", seed, 0, 0, B * N * N * EDGE_HIDDEN, P))
            out.append((f"model {B}x{N} layer {k} attention", seed, 1, 0, B * 2 * H * N * N, P))
    return out
