"""NumPy references and input builders for the dense sweep kernels (csrc/dense_sweeps.hip) and the
refinement aggregation (csrc/onegnn_refine.hip) -- TEST INFRASTRUCTURE, no GPU needed.

The references are the NumPy expressions the kernels reproduce (oracle/features_np.py where it has
them).  The builders put the extremum of a row or column where a strided loop, a tile tail or a
chunk boundary would lose it, and make every instance of a batch different."""
import numpy as np

from oracle import features_np

# (batch, n): one trip, two trips and more of the 256-thread loops; odd n (scalar column kernel), even n
# (16-byte pairs); 2048 x 2: one chunk through the batch term; 993 / 1025: last chunk of one row;
# 994: of two rows on the pair path; 514: a second column tile holding one pair
SHAPES = [(1, 1), (3, 2), (2048, 2), (5, 33), (3, 255), (3, 256), (3, 257), (2, 513), (2, 514), (1, 993),
          (1, 994), (1, 1025), (2, 1023)]
FAMILIES = ("uniform", "integer", "sparse", "negative", "signed_zero", "pos_inf", "neg_inf")
FINITE_FAMILIES = FAMILIES[:5]
SWEEP_THREADS = 256


def colmin_chunks(n, batch):
    """Row chunks of the column-minimum kernel, as the library's host code computes them."""
    coltiles = (n + 2 * SWEEP_THREADS - 1) // (2 * SWEEP_THREADS)
    chunks = (2048 + batch * coltiles - 1) // (batch * coltiles)
    return max(1, min(chunks, (n + 31) // 32))


def rows_per_chunk(n, batch):
    chunks = colmin_chunks(n, batch)
    return (n + chunks - 1) // chunks


def costs(family, batch, n, seed=0):
    """(batch, n, n) fp64 of one cost family; instances are drawn independently, so all differ."""
    rs = np.random.RandomState([seed, batch, n, FAMILIES.index(family)])
    shape = (batch, n, n)
    if family == "uniform":
        return rs.uniform(0.0, 1.0, shape)
    if family == "integer":
        return rs.randint(1, 10, shape).astype(np.float64)
    if family == "sparse":
        return np.where(rs.uniform(size=shape) < 0.7, 1e6, rs.uniform(0.0, 1.0, shape))
    if family == "negative":
        return -rs.uniform(1.0, 2.0, shape)
    if family == "signed_zero":
        return rs.choice(np.array([-0.0, 0.0, 0.5, 1.0]), size=shape)
    C = rs.uniform(0.0, 1.0, shape)
    C[rs.uniform(size=shape) < 0.1] = np.inf if family == "pos_inf" else -np.inf
    return C


def _floor(C):
    """A value below every finite entry of the batch, different per instance: (batch,)."""
    finite = C[np.isfinite(C)]
    lo = finite.min() if finite.size else 0.0
    return np.floor(lo) - 1.0 - np.arange(C.shape[0])


def row_plant_columns(n):
    return [j for j in (0, 255, 256, n - 1) if 0 <= j < n]


def col_plant_rows(n, batch):
    return sorted({0, min(rows_per_chunk(n, batch), n) - 1, n - 1})


def plant_row_minima(C):
    """Rows i with i % 3 != 2 get a strict minimum at one of the columns 0, 255, 256, n-1 (taking turns over
    rows and instances); the others keep what the family gave them.  Returns (C', columns) with columns
    (batch, n), -1 where nothing was planted."""
    C = C.copy()
    B, n, _ = C.shape
    cand = row_plant_columns(n)
    cols = np.full((B, n), -1)
    deep = _floor(C)
    for b in range(B):
        for i in range(n):
            if i % 3 != 2:
                cols[b, i] = cand[(i - i // 3 + b) % len(cand)]
                C[b, i, cols[b, i]] = deep[b]
    return C, cols


def plant_col_minima(C):
    """Columns j with j % 3 != 2 get a strict minimum at row 0, at the last row of the first chunk or at row
    n-1.  Returns (C', rows)."""
    C = C.copy()
    B, n, _ = C.shape
    cand = col_plant_rows(n, B)
    rows = np.full((B, n), -1)
    deep = _floor(C)
    for b in range(B):
        for j in range(n):
            if j % 3 != 2:
                rows[b, j] = cand[(j - j // 3 + b) % len(cand)]
                C[b, rows[b, j], j] = deep[b]
    return C, rows


def planted(family, batch, n, seed=0):
    """Costs with planted row minima, then planted column minima (a column plant may replace a row plant)."""
    C, _ = plant_row_minima(costs(family, batch, n, seed))
    return plant_col_minima(C)[0]


def small_duals(batch, n, seed=0):
    """(batch, n) N(0, 0.05): smaller than the depth of a planted minimum, different per instance."""
    return np.random.RandomState([seed, batch, n, 77]).normal(0.0, 0.05, (batch, n))


# ------------------------------------------------------------------------------- references
def quiet_errstate(fn):
    """inf - inf and NaN comparisons are part of what is tested; NumPy's warnings about them are not."""
    def wrapped(*a, **kw):
        with np.errstate(invalid="ignore", over="ignore"):
            return fn(*a, **kw)
    wrapped.__name__ = fn.__name__
    wrapped.__doc__ = fn.__doc__
    return wrapped


@quiet_errstate
def colmin(C, u=None):
    """(batch, n): min_i (C[b][i][j] - u[b][i]) through features_np.min_trick, one instance at a time."""
    if u is None:
        return C.min(axis=1)
    return np.stack([features_np.min_trick(C[b], u[b]) for b in range(C.shape[0])])


@quiet_errstate
def rowmin(C, v=None):
    return C.min(axis=-1) if v is None else (C - v[..., None, :]).min(axis=-1)


@quiet_errstate
def project_round(C, u, v):
    """One round of project_feasible, batched over the leading axis: (u', v', gmin)."""
    u1 = np.minimum(u, (C - v[..., None, :]).min(axis=-1))
    v1 = np.minimum(v, (C - u1[..., :, None]).min(axis=-2))
    gmin = ((C - u1[..., :, None]) - v1[..., None, :]).min(axis=(-2, -1))
    return u1, v1, gmin


@quiet_errstate
def reduce_costs(C, u, v, shift_nonneg):
    """(out, gmin) per instance: features_np.reduce_costs and the minimum of its unshifted matrix."""
    out = np.stack([features_np.reduce_costs(C[b], u[b], v[b], shift_nonneg) for b in range(C.shape[0])])
    gmin = np.stack([features_np.reduce_costs(C[b], u[b], v[b], False).min() for b in range(C.shape[0])])
    return out, gmin


def same(a, b):
    """Bit-for-bit in value: equal shapes, equal numbers, NaN exactly where the other has NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# --------------------------------------------------------------------------- seeds for the dual sweeps
@quiet_errstate
def project_seeds(C, seed=0, feasible=()):
    """Seeds as tests/golden/make_golden.py: make_features draws them, u = C.min(1) + N(0, 0.05), v = N(0, 0.05);
    the instances listed in `feasible` get u = rowmin(C - v) - 1/64 instead, which no round changes."""
    B, n, _ = C.shape
    rs = np.random.RandomState([seed, B, n, 78])
    u = C.min(axis=2) + rs.normal(0.0, 0.05, (B, n))
    v = rs.normal(0.0, 0.05, (B, n))
    for b in feasible:
        u[b] = (C[b] - v[b][None, :]).min(axis=1) - 0.015625
    return u, v


REDUCE_KINDS = ("negative", "zero", "positive")


@quiet_errstate
def reduce_seeds(C, shift=0, seed=0):
    """Instance b gets duals whose unshifted reduced minimum is negative, exactly 0 or positive, by
    (b + shift) % 3 (for finite C).  Returns (u, v, kinds)."""
    B, n, _ = C.shape
    rs = np.random.RandomState([seed, B, n, 79])
    u = np.empty((B, n))
    v = np.empty((B, n))
    kinds = []
    for b in range(B):
        kind = REDUCE_KINDS[(b + shift) % 3]
        noise_u, noise_v = rs.normal(0.0, 0.05, n), rs.normal(0.0, 0.05, n)
        if kind == "negative":
            u[b], v[b] = C[b].min(axis=1) + noise_u, noise_v
            u[b, 0] += 0.25  # whatever the noise drew
        elif kind == "zero":
            u[b] = C[b].min(axis=1) - np.abs(noise_u)
            v[b] = (C[b] - u[b][:, None]).min(axis=0)  # its argmin gives x - x, every other entry >= 0
        else:
            u[b], v[b] = C[b].min(axis=1) - 0.25, -np.abs(noise_v)
        kinds.append(kind)
    return u, v, kinds


# --------------------------------------------------------------------------- refinement aggregation
K = 16
REFINE_KINDS = ("full", "padded", "masked", "nonfinite", "ties", "spread_1e4", "spread_10", "full2")


def refine_inputs(rows, seed=0, shift=0, u_scale=1.0, u_offset=0.0, grid=False):
    """topk16 (rows, 16) float32 ascending and u_pre (rows,) float32.  Row r is of kind (r + shift) % 8:
    full finite; 1..15 trailing +inf (the padding of n < 16); all +inf (a masked row); a -inf and a NaN entry;
    16 equal values; steps of 1e4 (only the smallest survives exp) and of 10 (weights down to the float32
    denormals); full finite again.  `grid`: every number a small multiple of 2**-10, so that topk - u_pre is
    exact in float32 and in float64 alike."""
    rs = np.random.RandomState([seed, rows, shift, 80])
    top = np.sort(rs.uniform(0.0, 2.0, (rows, K)), axis=1)
    u = rs.normal(0.0, u_scale, rows) + u_offset
    kinds = []
    for r in range(rows):
        kind = REFINE_KINDS[(r + shift) % len(REFINE_KINDS)]
        if kind == "padded":
            top[r, K - 1 - (r // len(REFINE_KINDS) + shift) % 15:] = np.inf
        elif kind == "masked":
            top[r] = np.inf
        elif kind == "nonfinite":
            top[r, 0] = -np.inf
            top[r, 5] = np.nan
        elif kind == "ties":
            top[r] = top[r, 3]
        elif kind == "spread_1e4":
            top[r] = top[r, 0] + 1e4 * np.arange(K)
        elif kind == "spread_10":
            top[r] = top[r, 0] + 10.0 * np.arange(K)
        kinds.append(kind)
    if grid:
        with np.errstate(invalid="ignore"):
            top = np.round(top * 1024.0) / 1024.0
        u = np.round(u * 1024.0) / 1024.0
    return top.astype(np.float32), u.astype(np.float32), kinds


def refine_weights(H, seed=0, scale=1.0):
    rs = np.random.RandomState([seed, H, 81])
    return (rs.normal(0.0, scale, H).astype(np.float32), rs.normal(0.0, scale, H).astype(np.float32))


def refine_aggregate_ref(topk16, u_pre, w1, b1):
    """float64 restatement of lapwarm_refine_aggregate_batched: (out (rows, H), wsum (rows,)).
    val = float32(topk) - float32(u_pre) is formed in float32, as the kernel forms it; everything after it
    is float64: softmax(-val) over the finite entries, out = sum_k w_k GELU_erf(w1 val_k + b1)."""
    import torch
    with np.errstate(invalid="ignore", over="ignore"):
        val = (np.asarray(topk16, np.float32) - np.asarray(u_pre, np.float32)[:, None]).astype(np.float64)
        ok = np.isfinite(val)
        mn = np.where(ok, val, np.inf).min(axis=1, keepdims=True)
        e = np.where(ok, np.exp(-(np.where(ok, val, 0.0) - np.where(np.isfinite(mn), mn, 0.0))), 0.0)
        tot = e.sum(axis=1, keepdims=True)
        w = np.where(tot > 0, e / np.where(tot > 0, tot, 1.0), 0.0)
        x = (np.asarray(w1, np.float64)[None, None, :] * np.where(ok, val, 0.0)[:, :, None]
             + np.asarray(b1, np.float64)[None, None, :])
    xt = torch.from_numpy(x)
    gelu = (0.5 * xt * (1.0 + torch.erf(xt * 0.70710678118654752440))).numpy()
    return (w[:, :, None] * gelu).sum(axis=1), w.sum(axis=1)


def refine_aggregate_f32(topk16, u_pre, w1, b1):
    """The same formula in PyTorch-CPU float32, op for op as OneGNN._refine_reference_order before its second
    linear layer: what float32 arithmetic costs, the yardstick for the kernel's error."""
    import torch
    import torch.nn.functional as F
    base, up = torch.from_numpy(np.asarray(topk16, np.float32)), torch.from_numpy(np.asarray(u_pre, np.float32))
    values = base - up.unsqueeze(-1)
    valid = torch.isfinite(values)
    neg = torch.where(valid, -values, torch.full_like(values, -float("inf")))
    w = torch.softmax(neg, dim=-1)
    w = torch.where(valid, w, torch.zeros_like(w))
    e_in = torch.where(valid, values, torch.zeros_like(values)).unsqueeze(-1)
    e = F.gelu(F.linear(e_in, torch.from_numpy(w1).view(-1, 1), torch.from_numpy(b1)))
    return (w.unsqueeze(-1) * e).sum(dim=-2).numpy(), w.sum(dim=-1).numpy()
