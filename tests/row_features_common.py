"""Rows that each force one path of the row-feature kernel (csrc/dense_sweeps.hip: row_features_body, select_ranks)
at n = 1025 .. 16384, a NumPy restatement of the decisions that choose the path, and the tiling that makes an
n x n matrix out of a handful of rows.  No torch, no GPU: tests/test_row_features_host.py checks all of it on the
CPU, tests/test_gpu_row_features_large.py runs the rows through the kernels.

The restatement follows the kernel's comments, not its code:
  * first-level bucket of x in a row with minimum lo and maximum hi: trunc((x - lo) * 255 / (hi - lo)), clamped to
    0..255, 0 when hi == lo;
  * the three wanted ranks min(n, 16) - 1, (n - 1) >> 1 and n >> 1; the second selection, on |x - median| over
    [0, max |x - median|], wants the last two;
  * a bucket with more than 64 members is all-equal (recognised by a min / max reduction, no narrowing), or is
    narrowed by 8-bit passes over the IEEE order key from the top byte down until at most 64 members are left; what
    is still larger after the last byte is all-equal;
  * the order key of x: the bits of x + 0.0 (so -0.0 and +0.0 share one key), inverted for a negative x, with the
    sign bit set otherwise;
  * the entropy is summed element by element when some element has 0 < exp(-(x - lo)) < 1e-6 n, in closed form
    otherwise.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import features_np

# Dynamic LDS of one row workgroup: the workgroup exchange area (1552 bytes), npad = n rounded up to even doubles,
# the selection state (2976 bytes) and one bucket byte per element: 4528 + 9 npad.  It passes 64 KiB between
# n = 6778 (65530 bytes) and n = 6779 (npad = 6780: 65548 bytes) and is 151984 bytes at the cap, n = 16384.
LDS_FIXED = 1552 + 2976


def lds_bytes(n):
    npad = (n + 1) & ~1
    return LDS_FIXED + 9 * npad


LDS_BELOW = max(n for n in range(6000, 8000) if lds_bytes(n) <= 65536)
LDS_ABOVE = LDS_BELOW + 1
SIZES = (1025, 2048, 2049, 4096, 4097, LDS_BELOW, LDS_ABOVE, 16383, 16384)
LIST = 64  # what one wave ranks directly


def batch_of(n):
    """Instances per call of the comparison with NumPy: two while the matrices are small."""
    return 2 if n <= 4097 else 1


# ----------------------------------------------------------------------------------- the kernel's decisions
def order_key(x):
    b = (np.asarray(x, dtype=np.float64) + 0.0).view(np.int64)
    u = b.view(np.uint64)
    return np.where(b < 0, ~u, u | np.uint64(1 << 63))


def lin_bucket(x, lo, hi):
    width = hi - lo
    scale = 255.0 / width if 0.0 < width < np.inf else 0.0
    t = (np.asarray(x, dtype=np.float64) - lo) * scale
    bk = np.minimum(t, 255.0).astype(np.int64)
    return np.where(t > 0.0, bk, 0)


Target = namedtuple("Target", "rank bin count equal passes left below members")
Target.__doc__ = """One wanted rank of one selection: its first-level bucket and that bucket's member count; `equal`
is None, "first" (the bucket is all-equal as it stands) or "last" (all-equal after the last byte); `passes` narrowing
passes ran and left `left` members; `below` members of the bucket have a smaller key prefix than the target;
`members` are the indices of the first-level bucket's elements."""


def trace_select(vals, lo, hi, ranks):
    bk = lin_bucket(vals, lo, hi)
    key = order_key(vals)
    hist = np.bincount(bk, minlength=256)
    incl = np.cumsum(hist)
    out = []
    for r in ranks:
        b = int(np.searchsorted(incl, r, side="right"))
        kk = r - int(incl[b] - hist[b])
        members = np.flatnonzero(bk == b)
        cur = key[members]
        equal, passes, below, shift = None, 0, 0, 64
        if cur.size > LIST and cur.min() == cur.max():
            equal = "first"
        else:
            while cur.size > LIST:
                if shift == 0:
                    equal = "last"
                    break
                byte = ((cur >> np.uint64(shift - 8)) & np.uint64(255)).astype(np.int64)
                h = np.bincount(byte, minlength=256)
                c = np.cumsum(h)
                t = int(np.searchsorted(c, kk, side="right"))
                before = int(c[t] - h[t])
                kk -= before
                below += before
                cur = cur[byte == t]
                shift -= 8
                passes += 1
        out.append(Target(r, b, int(members.size), equal, passes, int(cur.size), below, members))
    return out, int(incl[out[0].bin] - hist[out[0].bin]) + out[0].below


RowTrace = namedtuple("RowTrace", "first mad lowcount elementwise median")
RowTrace.__doc__ = """first: the three targets of the selection on the row; mad: the two of the selection on
|x - median|; lowcount: how many elements the top-16 gather finds below target 0's final bucket; elementwise: the
entropy takes the element-by-element pass."""


def trace_row(x):
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    lo, hi = x.min(), x.max()
    ranks = (min(n, 16) - 1, (n - 1) >> 1, n >> 1)
    first, lowcount = trace_select(x, lo, hi, ranks)
    srt = np.sort(x)
    med = srt[n >> 1] if n & 1 else (srt[(n - 1) >> 1] + srt[n >> 1]) / 2.0
    assert med == np.median(x)
    dev = np.abs(x - med)
    mad, _ = trace_select(dev, 0.0, max(abs(lo - med), abs(hi - med)), ranks[1:])
    e = np.exp(-(x - lo))
    return RowTrace(first, mad, lowcount, bool(((e > 0.0) & (e < 1e-6 * n)).any()), med)


def describe(tr):
    """One line for the profile note: what each target of a traced row went through."""
    def one(t):
        if t.count <= LIST:
            return f"{t.count}"
        if t.equal == "first":
            return f"{t.count} all-equal"
        tail = " then all-equal at the last byte" if t.equal == "last" else ""
        return f"{t.count} -> {t.left} in {t.passes} passes{tail}"
    return ("row: " + "; ".join(one(t) for t in tr.first) + f" | lowcount {tr.lowcount} | MAD: "
            + "; ".join(one(t) for t in tr.mad) + " | entropy " + ("element-wise" if tr.elementwise else "closed form"))


# ----------------------------------------------------------------------------------------------- the recipes
def _rng(tag, n):
    return np.random.default_rng([tag, n])


def _narrowed(t):
    return t.count > LIST and t.equal is None and t.passes >= 1 and t.left <= LIST


def _quiet(t):
    return t.count <= LIST


# uniform: 256 buckets of n / 256 expected members.  Up to n = 6779 (26 per bucket) no target's bucket passes 64 in
# either selection; at 16383 and 16384 (64 per bucket) some target's bucket does, for the rows of these seeds.
UNIFORM_IS_QUIET = {1025: True, 2048: True, 2049: True, 4096: True, 4097: True, LDS_BELOW: True, LDS_ABOVE: True,
                    16383: False, 16384: False}


def row_uniform(n):
    return _rng(1, n).random(n)


def holds_uniform(x):
    tr = trace_row(x)
    return all(_quiet(t) for t in tr.first + tr.mad) == UNIFORM_IS_QUIET[x.size]


def row_outlier(n):
    """uniform [0, 1) and one element at 1e12: every other element is in bucket 0."""
    rng = _rng(2, n)
    x = rng.random(n)
    x[rng.integers(n)] = 1e12
    return x


def holds_outlier(x):
    tr = trace_row(x)
    return all(t.bin == 0 and t.count == x.size - 1 and _narrowed(t) for t in tr.first)


CLUSTER_GROUP = 40
ONE_BITS = int(np.float64(1.0).view(np.uint64))
K1_BITS = int(np.float64(2.0 ** 9).view(np.uint64))  # x 2^40 = 2^49: exponent 0x430, byte 2 of the key is 0
SCALE = 2.0 ** 40


def _in_the_middle(n, cluster, rng, outer=1.0):
    """`cluster` (more than n / 2 values) with 20 to 59 elements of outer x [-200, -100) below it and the rest, in
    outer x [100, 200], above: -200 and 200 are present and bucket 127 or 128 of the 256 holds the cluster alone.
    The median is in the cluster and nearly everything below it is too, so that the median of |x - median| is the
    distance from the median to one element near the cluster's lower end: it moves by as much as the median does.
    For an even n the count below puts the two middle elements 40 j - 1 and 40 j places into the cluster.  The row
    is then scaled by 2^40, which moves no element to another bucket and leaves every mantissa as it was, so that
    differences inside the cluster (down to one ulp) are far above the 1e-9 floor of column 4 and show in its
    float32 value."""
    m = cluster.size
    nlo = 20 + (n // 2 - 20) % CLUSTER_GROUP
    assert 2 * m > n
    low = outer * (-200.0 + 100.0 * rng.random(nlo))
    high = outer * (100.0 + 100.0 * rng.random(n - m - nlo))
    low[0], high[0] = -200.0 * outer, 200.0 * outer
    return SCALE * rng.permutation(np.concatenate([low, cluster, high]))


LATTICE_EXTRA = 13


def cluster_groups(n):
    return n // (2 * CLUSTER_GROUP) + 1  # more than n / 2 values; 205 of a byte's 256 at n = 16384


def row_cluster(k, n, tag=10):
    """More than half the row around the median: (1 + (q 2^(56 - 8k) + r) ulp) with q = 0, 1, .. (40 values each) and
    r < 2^(56 - 8k) random.  Their keys agree in the top 8 k bits and q sits in the next byte, so k passes leave the
    whole cluster and pass k + 1 leaves the 40 of one q.  k = 7 splits on the last byte, the 40 of a q being
    bit-equal; its q = 0 has 13 more, without which the values and the ranks would step together and column 4 of
    an even n, the mean of two neighbouring ranks, would hide half an ulp of the median.  k = 1 starts at 2^9, not 1 (byte 2 of the scaled key is then 0), and spans 2^9 .. 2^22."""
    rng = _rng(tag + k, n)
    sh = 56 - 8 * k
    q = np.repeat(np.arange(cluster_groups(n), dtype=np.uint64), CLUSTER_GROUP)
    q = np.concatenate([np.zeros(LATTICE_EXTRA if k == 7 else 0, dtype=np.uint64), q])
    r = rng.integers(0, 1 << sh, q.size, dtype=np.uint64) if sh else np.zeros(q.size, dtype=np.uint64)
    bits = np.uint64(K1_BITS if k == 1 else ONE_BITS) + (q << np.uint64(sh)) + r
    return _in_the_middle(n, bits.view(np.float64), rng, outer=2.0 ** 25 if k == 1 else 1.0)


def holds_cluster(k, x):
    tr = trace_row(x)
    ok = True
    for t in tr.first[1:]:
        keys = order_key(x[t.members])
        agree = 64 - int(keys.min() ^ keys.max()).bit_length()
        size = cluster_groups(x.size) * CLUSTER_GROUP + (LATTICE_EXTRA if k == 7 else 0)
        ok = ok and t.count == size and 8 * k <= agree < 8 * k + 8
        ok = ok and t.equal is None and t.passes == k + 1 and t.left == CLUSTER_GROUP
    return ok and all(t.count > x.size // 2 for t in tr.mad)


def row_negative_cluster(n):
    """cluster_3 with every sign changed: the passes run over inverted keys."""
    return -row_cluster(3, n, tag=30)


def holds_negative_cluster(x):
    return holds_cluster(3, x) and all((x[t.members] < 0.0).all() for t in trace_row(x).first[1:])


def row_cluster_equal(n):
    """n / 2 + 140 copies of one value around the median between 60 values just below and 60 just above it (up to
    2^30 ulp away): the bucket is not all-equal, every narrowing pass runs, and more than 64 bit-equal values are
    left after the last byte.  |x - median| is 0 for more than half the row, so the second selection ends the same
    way and column 4 is its floor, 1e-9, unless the median is another value than the repeated one."""
    rng = _rng(20, n)
    one = np.uint64(ONE_BITS)
    under = one - np.uint64(1) - rng.integers(0, 1 << 30, 60, dtype=np.uint64)
    over = one + np.uint64(1) + rng.integers(0, 1 << 30, 60, dtype=np.uint64)
    bits = np.concatenate([under, np.full(n // 2 + 140, one, dtype=np.uint64), over])
    return _in_the_middle(n, bits.view(np.float64), rng)


def holds_cluster_equal(x):
    tr = trace_row(x)
    copies = x.size // 2 + 140
    return all(t.count == copies + 120 and t.equal == "last" and t.passes == 8 and t.left == copies
               for t in tr.first[1:] + tr.mad)


def row_ties_low(n):
    """Bucket 0 of a row over [2^-40, 1000] holds 7 values near 2^-40, 200 values 2^-10 (1 + i / 32) with ties, and
    whatever else is below 3.92.  Rank 15 is among the 200; their key prefix is above that of the 7."""
    rng = _rng(3, n)
    tiny = 2.0 ** -40 * (1.0 + np.arange(7) / 8.0)
    mid = 2.0 ** -10 * (1.0 + rng.integers(0, 32, 200) / 32.0)
    rest = 1.0 + 999.0 * rng.random(n - 207)
    rest[0] = 1000.0
    return rng.permutation(np.concatenate([tiny, mid, rest]))


def holds_ties_low(x):
    tr = trace_row(x)
    t = tr.first[0]
    tied = np.unique(np.sort(x)[:16]).size < 16
    return t.bin == 0 and _narrowed(t) and t.below >= 1 and 1 <= tr.lowcount <= 15 and tied


def row_two_clusters(n):
    """Half the row in [0.05, 0.051], half in [0.949, 0.95]; 24 sparse elements at each end and 24 around 0.5 keep
    the targets of the first selection in buckets of a few.  |x - median| puts both halves at 0.45."""
    rng = _rng(4, n)
    s = 24
    bottom = 0.04 * rng.random(s)
    top = 1.0 - 0.04 * rng.random(s)
    bottom[0], top[0] = 0.0, 1.0
    off = np.concatenate([[1e-4], 0.002 + 0.038 * rng.random(s // 2 - 1)])
    middle = np.concatenate([0.5 - off, 0.5 + off])
    m = n - 3 * s
    lowc = 0.05 + 0.001 * rng.random(m // 2)
    highc = 0.95 - 0.001 * rng.random(m - m // 2)
    return rng.permutation(np.concatenate([bottom, top, middle, lowc, highc]))


def holds_two_clusters(x):
    tr = trace_row(x)
    ok = all(_quiet(t) for t in tr.first)
    for t in tr.mad:
        side = x[t.members] < tr.median
        ok = ok and _narrowed(t) and side.sum() > LIST and (~side).sum() > LIST
    return ok


def row_constant(n):
    """The integer family, 0..9: from n = 1025 on every value has more than 64 copies and a bucket of its own."""
    return _rng(5, n).integers(0, 10, n).astype(np.float64)


def holds_constant(x):
    tr = trace_row(x)
    return np.bincount(x.astype(np.int64), minlength=10).min() > LIST and all(t.equal == "first" for t in tr.first + tr.mad)


def row_signed(n):
    """Around the median: 50 values -2^-e and 50 values 2^-e (30 <= e < 1000), -5e-324, -2.5e-310, -0.0, +0.0,
    5e-324, 2.5e-310; the rest exponential on both sides of zero.  The median's bucket holds both signs, both
    zeros and the subnormals, and is narrowed on keys of both signs."""
    rng = _rng(6, n)
    neg = -(2.0 ** -rng.integers(30, 1000, 50).astype(np.float64))
    pos = 2.0 ** -rng.integers(30, 1000, 50).astype(np.float64)
    tiny = np.concatenate([neg, pos, [-5e-324, -2.5e-310, -0.0, 0.0, 5e-324, 2.5e-310]])
    nlo = (n - tiny.size) // 2
    low = -(0.01 + rng.exponential(1.0, nlo))
    high = 0.01 + rng.exponential(1.0, n - tiny.size - nlo)
    return rng.permutation(np.concatenate([low, tiny, high]))


def holds_signed(x):
    tr = trace_row(x)
    ok = x.min() < 0.0 and tr.median == 0.0
    for t in tr.first[1:]:
        v = x[t.members]
        zeros = v[v == 0.0]
        sub = v[(v != 0.0) & (np.abs(v) < 2.0 ** -1022)]
        ok = ok and _narrowed(t) and (v < 0).any() and (v > 0).any() and sub.size == 4
        ok = ok and np.signbit(zeros).any() and not np.signbit(zeros).all()
    return ok


ENTROPY_AT_LO = 64


def row_entropy_edge(n, side, tau_n=None):
    """64 elements at lo = 0 (e = 1), one with e = exp(-x) a factor 1 +- 2^-20 from 1e-6 tau_n, every other
    element at 1e4 or more (e = 0 exactly).  tau_n = n: "above" is closed-form, "below" element-wise.  The "below"
    row of tau_n = 4096 at n = 257 is the same content under a threshold 16 times smaller: closed-form there."""
    tau_n = n if tau_n is None else tau_n
    rng = _rng(7 if side == "above" else 8, n)
    e = 1e-6 * tau_n * (1.0 + (2.0 ** -20 if side == "above" else -(2.0 ** -20)))
    far = 1e4 * (1.0 + rng.random(n - ENTROPY_AT_LO - 1))
    return rng.permutation(np.concatenate([np.zeros(ENTROPY_AT_LO), [-np.log(e)], far]))


def holds_entropy_edge(x, elementwise, tau_n=None):
    """One element with 0 < e < 1, within 2^-19 of the threshold of tau_n; the row takes the stated branch."""
    e = np.exp(-(x - x.min()))
    between = (e > 0.0) & (e < 1.0)
    tau = 1e-6 * (x.size if tau_n is None else tau_n)
    return (between.sum() == 1 and (e == 1.0).sum() == ENTROPY_AT_LO and abs(e[between][0] / tau - 1.0) < 2.0 ** -19
            and trace_row(x).elementwise == elementwise)


Recipe = namedtuple("Recipe", "name row holds path")
RECIPES = (
    Recipe("uniform", row_uniform, holds_uniform, "control: no bucket above 64 up to n = 6779"),
    Recipe("outlier", row_outlier, holds_outlier, "all three targets narrow out of bucket 0"),
    Recipe("cluster_1", functools.partial(row_cluster, 1), functools.partial(holds_cluster, 1), "2 passes"),
    Recipe("cluster_3", functools.partial(row_cluster, 3), functools.partial(holds_cluster, 3), "4 passes"),
    Recipe("cluster_6", functools.partial(row_cluster, 6), functools.partial(holds_cluster, 6), "7 passes"),
    Recipe("cluster_7", functools.partial(row_cluster, 7), functools.partial(holds_cluster, 7),
           "8 passes: the last byte"),
    Recipe("negative_cluster", row_negative_cluster, holds_negative_cluster, "4 passes over inverted keys"),
    Recipe("ties_low", row_ties_low, holds_ties_low, "the `below` branch of the top-16 gather, lowcount 1..15"),
    Recipe("two_clusters", row_two_clusters, holds_two_clusters, "only the MAD selection narrows"),
    Recipe("constant", row_constant, holds_constant, "every bucket all-equal, more than 64 copies"),
    Recipe("signed", row_signed, holds_signed, "negative keys, -0.0 / +0.0, subnormals in the median's bucket"),
    Recipe("entropy_above", lambda n: row_entropy_edge(n, "above"), lambda x: holds_entropy_edge(x, False),
           "closed-form entropy, e just above 1e-6 n"),
    Recipe("entropy_below", lambda n: row_entropy_edge(n, "below"), lambda x: holds_entropy_edge(x, True),
           "element-wise entropy, e just below 1e-6 n"),
    # last: the row that a tiled matrix holds once
    Recipe("cluster_equal", row_cluster_equal, holds_cluster_equal,
           "all 8 passes, then more than 64 equal values at shift 0"),
)
NAMES = tuple(r.name for r in RECIPES)


# ------------------------------------------------------------------------------------------------- tiling
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def base_rows(n):
    """(R, n): one row per recipe.  Then one column minimum is made to be attained by two rows: in a column whose
    minimum cluster_3 holds with one of its elements of 2^40 x (-200, -100), cluster_6 gets an element of its own
    from that range (two of its elements change places) and this element is set to cluster_3's value.  As a
    multiset cluster_6 changes in one element, which stays inside the range of its lowest part, below rank 20."""
    base = np.stack([r.row(n) for r in RECIPES])
    a, b = NAMES.index("cluster_3"), NAMES.index("cluster_6")

    def low_part(x):
        return (x > -200.0 * SCALE) & (x < -100.0 * SCALE)
    j = int(np.flatnonzero((base.argmin(axis=0) == a) & low_part(base[a]))[0])
    j2 = int(np.flatnonzero(low_part(base[b]))[0])
    base[b, j2] = base[b, j]
    base[b, j] = base[a, j]
    return _frozen(base)


def entropy_rows(n):
    """(3, n): the two edge rows of n, and the below-threshold row of n = 4096 at this n."""
    return _frozen(np.stack([row_entropy_edge(n, "above"), row_entropy_edge(n, "below"),
                             row_entropy_edge(n, "below", tau_n=4096)]))


def tile_index(n, R, shift=0):
    """Which base row is row i of the tiled matrix: rows 0 .. n-2 cycle through the first R - 1 base rows, starting
    at `shift`, and the last base row is row n - 1 alone.  Needs n >= R."""
    assert n >= R >= 2
    return np.concatenate([(np.arange(n - 1) + shift) % (R - 1), [R - 1]])


INSTANCE_SHIFT = (0, 5)


def instance_rows(base, b):
    """Instance 0 is tiled from the base rows; instance 1 from their mirror images (columns reversed), in another
    order (tile_index's shift).  A row and its mirror image have the same statistics, but the column minima of the
    two instances are each other's mirror images, so column 12 of one instance, counted against the minima of the
    other, comes out wrong."""
    return base if b == 0 else np.ascontiguousarray(base[:, ::-1])


Expected = namedtuple("Expected", "stats feat32 topk32")


def expected_rows(rows):
    """The reference on the R rows alone: columns 0-11 and the top-16 depend on the row alone; column 12 counts the
    column minima of the matrix, which are those of the R rows because every one of them occurs in it."""
    stats = features_np.row_statistics(rows)
    return Expected(_frozen(stats), _frozen(stats.astype(np.float32)),
                    _frozen(features_np.topk_smallest(rows).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def expected(n, b):
    return expected_rows(instance_rows(base_rows(n), b))


EXACT_COLUMNS = (0, 1, 4, 6, 11, 12)
RTOL, ATOL = 3e-6, 1e-9  # test_row_features_batched's


def column_errors(got, want):
    """Largest |got - want| / |want| per column (0 where both are 0), 13 values."""
    got, want = got.astype(np.float64), want.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(got - want) / np.abs(want)
    rel[got == want] = 0.0
    return rel.max(axis=0)
