"""The draw rules and the seven synthetic cost families of csrc/cost_families.hpp restated in NumPy on the Philox words
of dual_dropout_common, and the cases and seeds that the tests use -- TEST INFRASTRUCTURE, no GPU needed.

Every value is a pure function of (seed, stream, element): key (lo32(seed), hi32(seed)), counter (lo32(group),
hi32(group), stream, 0).
  dbl(hi, lo) = ((hi >> 5) 2^26 + (lo >> 6)) 2^-53
  U_s(e): group e >> 1, dbl(w[2 (e & 1)], w[2 (e & 1) + 1])
  Z_s(e): group e >> 1, u1 = dbl(w0, w1), u2 = dbl(w2, w3), r = sqrt(-2 log(1 - u1)), t = 6.283185307179586 u2,
          r cos(t) for even e, r sin(t) for odd e
  I_s(e, m) = (w[e & 3] of group e >> 2) m >> 32
A matrix is built from a `normals(stream, count)` callable that gives Z of the elements 0 .. count - 1 of a stream: the
GPU tests hand in the device's own draws, so that its libm is compared once (the draws test) and every other operation
of a family is checked to the bit; the host tests hand in `normals_numpy`.  Sums over the rank run in explicit
ascending-k loops of elementwise operations, each rounded."""
import math

import numpy as np

from dual_dropout_common import philox4x32_10

U0, Z1, FACTOR_A, FACTOR_B, MASK, REPAIR = range(6)
FAMILY_IDS = {"uniform": 0, "metric": 1, "low_rank": 2, "clustered": 3, "noisy_linear": 4, "tie": 5, "sparse": 6}
DEFAULTS = {"uniform": (0, 0.0), "metric": (0, 0.0), "low_rank": (12, 0.1), "clustered": (4, 0.1),
            "noisy_linear": (1, 0.1), "tie": (5, 1e-6), "sparse": (0, 0.3)}
TILE_ROWS, TILE_COLS = 8, 128   # kCostTileRows, kCostTileCols
SPARSE_FILL = 1e6
_LO, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def words(seed, stream, groups):
    """(len(groups), 4) uint64: the four words of every group."""
    seed = int(seed)
    assert 0 <= seed < 2**64
    g = np.asarray(groups, dtype=np.uint64)
    return np.stack(philox4x32_10((g & _LO, g >> _32, stream, 0), (seed & 0xFFFFFFFF, seed >> 32)), axis=-1)


def dbl(hi, lo):
    return ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64)) * 2.0**-53


def _pairs(first, count):
    """The groups that hold the elements first .. first + count - 1 two to a group, and where the first one sits."""
    g0, g1 = first >> 1, (first + count - 1) >> 1
    return np.arange(g0, g1 + 1, dtype=np.uint64), first - 2 * g0


def uniforms(seed, stream, first, count):
    g, at = _pairs(int(first), int(count))
    w = words(seed, stream, g)
    u = np.stack((dbl(w[:, 0], w[:, 1]), dbl(w[:, 2], w[:, 3])), axis=-1).reshape(-1)
    return u[at:at + count]


def normals_numpy(seed, stream, first, count):
    """Z in plain float64 NumPy: the conditions of the host tests."""
    g, at = _pairs(int(first), int(count))
    w = words(seed, stream, g)
    u1, u2 = dbl(w[:, 0], w[:, 1]), dbl(w[:, 2], w[:, 3])
    r = np.sqrt(-2.0 * np.log(1.0 - u1))
    t = 6.283185307179586 * u2
    return np.stack((r * np.cos(t), r * np.sin(t)), axis=-1).reshape(-1)[at:at + count]


def normals_reference(seed, stream, first, count):
    """Z with every operation after the exact ones (1 - u1, the product with the double 6.283185307179586) carried
    wider than double and rounded to double once: np.longdouble where it has more than 53 bits, else exact rational
    arguments through math.log / math.cos / math.sin (correct to well under 1 ulp)."""
    g, at = _pairs(int(first), int(count))
    w = words(seed, stream, g)
    u1, u2 = dbl(w[:, 0], w[:, 1]), dbl(w[:, 2], w[:, 3])
    if np.finfo(np.longdouble).nmant > 52:
        L = np.longdouble
        r = np.sqrt(L(-2.0) * np.log(L(1.0) - u1.astype(L)))
        t = L(6.283185307179586) * u2.astype(L)
        z = np.stack((r * np.cos(t), r * np.sin(t)), axis=-1).astype(np.float64)
    else:
        z = np.array([[math.sqrt(-2.0 * math.log(1.0 - a)) * math.cos(6.283185307179586 * b),
                       math.sqrt(-2.0 * math.log(1.0 - a)) * math.sin(6.283185307179586 * b)] for a, b in zip(u1, u2)])
    return z.reshape(-1)[at:at + count]


def integers(seed, stream, first, count, m):
    first, count = int(first), int(count)
    g0, g1 = first >> 2, (first + count - 1) >> 2
    w = words(seed, stream, np.arange(g0, g1 + 1, dtype=np.uint64)).reshape(-1)
    at = first - 4 * g0
    return ((w[at:at + count] * np.uint64(m)) >> _32).astype(np.int64)


def clamp(x):
    return np.where(x > 0.0, x, 0.0)


def factor_sum(a, b, rank):
    S = np.zeros((a.shape[0], b.shape[0]))
    for k in range(rank):
        S = S + a[:, k][:, None] * b[:, k][None, :]
    return S


def sparse_keep(n, seed, sparsity):
    """keep (n, n) after the repairs, the rows that were repaired and the columns that were repaired after them."""
    keep = (uniforms(seed, MASK, 0, n * n) < sparsity).reshape(n, n)
    rows = [i for i in range(n) if not keep[i].any()]
    for i in rows:
        keep[i, int(integers(seed, REPAIR, i, 1, n)[0])] = True
    cols = [j for j in range(n) if not keep[:, j].any()]
    for j in cols:
        keep[int(integers(seed, REPAIR, n + j, 1, n)[0]), j] = True
    return keep, rows, cols


def matrix(family, n, seed, p0=None, p1=None, normals=None):
    """The n x n matrix of `family`; p0, p1 default to the reference's; normals(stream, count) -> Z of a stream."""
    d0, d1 = DEFAULTS[family]
    p0, p1 = d0 if p0 is None else int(p0), d1 if p1 is None else float(p1)
    if normals is None:
        normals = lambda stream, count: normals_numpy(seed, stream, 0, count)  # noqa: E731
    nn = n * n
    if family == "uniform":
        return uniforms(seed, U0, 0, nn).reshape(n, n)
    if family == "metric":
        p = (100.0 * uniforms(seed, U0, 0, 2 * n)).reshape(n, 2)
        dx, dy = p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]
        return np.sqrt(dx * dx + dy * dy)
    if family in ("low_rank", "noisy_linear"):
        a = normals(FACTOR_A, n * p0).reshape(n, p0)
        b = normals(FACTOR_B, n * p0).reshape(n, p0)
        T = factor_sum(a, b, p0) + p1 * normals(Z1, nn).reshape(n, n)
        return clamp(T) if family == "low_rank" else T - T.min()
    if family == "clustered":
        size = max(1, n // max(1, p0))
        blk = np.minimum(np.arange(n) // size, p0 - 1)
        same = blk[:, None] == blk[None, :]
        u = uniforms(seed, U0, 0, nn).reshape(n, n)
        return clamp((u - np.where(same, 0.4, 0.0)) + p1 * normals(Z1, nn).reshape(n, n))
    if family == "tie":
        m = max(1, p0)
        base = integers(seed, MASK, 0, nn, m).astype(np.float64) / float(m)
        return (base + p1 * uniforms(seed, U0, 0, nn)).reshape(n, n)
    assert family == "sparse"
    keep, _, _ = sparse_keep(n, seed, p1)
    return np.where(keep, uniforms(seed, U0, 0, nn).reshape(n, n), SPARSE_FILL)


# ---- the cases of tests/test_gpu_cost_families.py ---------------------------------------------------------------

SEED_DRAWS = 0x8000_0000_0000_0000 | 0x0BAD_5EED_1234   # bit 63 set
DRAWS_FIRST, DRAWS_COUNT = 2**34 + 5, 4099              # not a multiple of 4, past 2^34
SIZES = (1, 2, 3, 7, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, TILE_COLS - 1, TILE_COLS, TILE_COLS + 1)
# sparse at n in 3..8: seeds searched on the CPU (search_sparse_seed) so that a row repair and, after it, a column
# repair happen; test_cost_families_host.py holds them to that
SPARSE_SEEDS = {3: 5, 7: 4, 8: 4}


def search_sparse_seed(n, sparsity=0.3, limit=4096):
    for seed in range(limit):
        _, rows, cols = sparse_keep(n, seed, sparsity)
        if rows and cols:
            return seed
    raise AssertionError(n)


def case_seed(family, n, k):
    if family == "sparse" and n in SPARSE_SEEDS:
        return SPARSE_SEEDS[n]
    return (0x9E37_79B9_7F4A_7C15 * (k + 1) + 1000003 * FAMILY_IDS[family] + n) % 2**64


def cases():
    """[(family, n, seed, p0, p1)]: every family at every size of SIZES with its defaults, then the other
    parameters: rank 1 and 64, blocks 1 and n + 3, bins 1."""
    out = []
    for family in FAMILY_IDS:
        for n in sorted(set(SIZES)):
            out.append((family, n, case_seed(family, n, len(out)), *DEFAULTS[family]))
    for family, n, p0 in (("low_rank", 9, 1), ("low_rank", 9, 64), ("noisy_linear", 7, 12), ("noisy_linear", 9, 64),
                          ("clustered", 9, 1), ("clustered", 9, 12), ("clustered", 129, 132), ("tie", 9, 1)):
        out.append((family, n, case_seed(family, n, len(out)), p0, DEFAULTS[family][1]))
    return out


# the mixed batch: five families, distinct sizes, an odd size before another instance (the next one starts 8 bytes
# off a 16-byte boundary), and one instance of size 0 that gets no work
MIXED = (("metric", 7, 101), ("sparse", 9, 102), ("low_rank", 129, 103), ("uniform", 0, 104), ("noisy_linear", 8, 105),
         ("tie", 3, 106))
