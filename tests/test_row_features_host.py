"""tests/row_features_common.py on the CPU: every row that tests/test_gpu_row_features_large.py sends through the
row-feature kernel takes the path it is there for (by the NumPy restatement of the kernel's decisions), the
reference is finite on it, and the expectation of a tiled matrix, computed from its distinct rows alone, is what the
reference gives on the whole matrix."""
import numpy as np
import pytest

import row_features_common as rfc
from oracle import features_np


@pytest.mark.parametrize("n", rfc.SIZES)
def test_every_recipe_takes_its_path(n):
    base = rfc.base_rows(n)
    assert base.shape == (len(rfc.RECIPES), n) and np.isfinite(base).all()
    for r, x in zip(rfc.RECIPES, base):
        assert bool(r.holds(x)), (r.name, n, rfc.describe(rfc.trace_row(x)))


def test_sizes_straddle_the_lds_and_the_list_thresholds():
    assert rfc.lds_bytes(rfc.LDS_BELOW) <= 65536 < rfc.lds_bytes(rfc.LDS_ABOVE) and rfc.LDS_ABOVE in rfc.SIZES
    assert rfc.lds_bytes(16384) <= 160 * 1024
    # the control narrows nowhere while n / 256 is small, and does at the cap: both truth values occur
    assert set(rfc.UNIFORM_IS_QUIET) == set(rfc.SIZES) and set(rfc.UNIFORM_IS_QUIET.values()) == {True, False}


def test_paths_that_need_two_targets_occur():
    """One target narrows while another of the same selection does not (the gather then computes keys for members
    that need none), and the two median targets end in different final buckets."""
    tr = rfc.trace_row(rfc.base_rows(1025)[rfc.NAMES.index("cluster_3")])
    assert tr.first[0].count <= rfc.LIST and tr.first[1].passes == 4
    tr = rfc.trace_row(rfc.base_rows(1025)[rfc.NAMES.index("ties_low")])
    assert tr.first[0].passes >= 1 and tr.first[1].count <= rfc.LIST
    for n in (2048, 16384):  # even: the two middle elements are the last of one group of 40 and the first of the next
        x = rfc.base_rows(n)[rfc.NAMES.index("cluster_6")]
        lo_mid, hi_mid = np.sort(x)[[(n - 1) >> 1, n >> 1]]
        assert rfc.order_key(lo_mid) >> np.uint64(8) != rfc.order_key(hi_mid) >> np.uint64(8)


@pytest.mark.parametrize("n", (1025, 2048, 16384))
def test_a_wrong_median_shows_in_column_4(n):
    """The median itself is no output; column 4, the median of |x - median|, is.  For the rows whose point is the
    selection of the median out of a narrowed bucket, taking the next distinct value on either side of a middle
    element in its place changes the float32 value of column 4."""
    for name in ("cluster_1", "cluster_3", "cluster_6", "cluster_7", "negative_cluster", "cluster_equal"):
        x = rfc.base_rows(n)[rfc.NAMES.index(name)]
        srt = np.unique(x)
        right = np.float32(features_np.row_statistics(x[None])[0, 4])
        middle = np.sort(x)[[(n - 1) >> 1, n >> 1]]
        for i in (0, 1):
            at = int(np.searchsorted(srt, middle[i]))
            for wrong in (srt[at - 1], srt[at + 1]):
                taken = middle.copy()
                taken[i if n % 2 == 0 else slice(None)] = wrong
                median = (taken[0] + taken[1]) / 2.0
                if median == np.median(x):  # one ulp in one of two elements, rounded away by the mean
                    continue
                mad = max(np.median(np.abs(x - median)), features_np.EPS)
                assert np.float32(mad) != right, (name, n, i, mad, right)


def test_order_key_orders_like_the_values():
    x = rfc.base_rows(1025)[rfc.NAMES.index("signed")]
    srt = np.sort(x)
    keys = rfc.order_key(srt)
    assert (np.diff(keys.astype(object)) >= 0).all()
    assert rfc.order_key(-0.0) == rfc.order_key(0.0)
    assert rfc.order_key(-5e-324) < rfc.order_key(0.0) < rfc.order_key(5e-324)


@pytest.mark.parametrize("n", (257, 4096))
def test_entropy_rows_sit_on_both_sides_of_the_threshold(n):
    above, below, of4096 = rfc.entropy_rows(n)
    assert bool(rfc.holds_entropy_edge(above, False)) and bool(rfc.holds_entropy_edge(below, True))
    # the same content (64 elements at lo, one with e just below 4.096e-3, e == 0 elsewhere) at both sizes
    assert bool(rfc.holds_entropy_edge(of4096, n == 4096, tau_n=4096))
    assert np.array_equal(np.sort(of4096)[:65], np.sort(rfc.entropy_rows(4096)[2])[:65])
    assert np.isfinite(rfc.expected_rows(rfc.entropy_rows(n)).stats).all()


@pytest.mark.parametrize("n", rfc.SIZES)
def test_reference_is_finite_and_column_12_is_not_trivial(n):
    base = rfc.base_rows(n)
    for b in range(rfc.batch_of(n)):
        rows = rfc.instance_rows(base, b)
        want = rfc.expected(n, b)
        assert np.isfinite(want.stats).all() and np.isfinite(want.topk32).all()
        colmin = rows.min(axis=0)
        holders = (rows == colmin).sum(axis=0)
        assert (holders == 2).any(), "no column minimum attained by two base rows"
        once = (rows[-1] == colmin) & (holders == 1)
        assert once.any(), "the row that occurs once holds no column minimum of its own"
        col12 = want.stats[:, 12]
        assert len({float(c) for c in col12} - {0.0, 1.0 / n}) >= 4, col12
    if rfc.batch_of(n) == 2:
        # counted against the other instance's minima, column 12 differs: a mix-up shows
        mirrored = features_np.row_statistics(rfc.instance_rows(base, 1), col_min=base.min(axis=0))
        assert (mirrored[:, 12] != rfc.expected(n, 1).stats[:, 12]).sum() >= 4


@pytest.mark.parametrize("b", (0, 1))
def test_tiled_expectation_is_the_reference_on_the_whole_matrix(b):
    n = 1025
    rows = rfc.instance_rows(rfc.base_rows(n), b)
    idx = rfc.tile_index(n, rows.shape[0], rfc.INSTANCE_SHIFT[b])
    assert idx[-1] == rows.shape[0] - 1 and (idx[:-1] < rows.shape[0] - 1).all()
    assert (np.bincount(idx)[:-1] >= 2).all() and np.bincount(idx)[-1] == 1
    C = rows[idx]
    want = rfc.expected(n, b)
    assert np.array_equal(features_np.row_statistics(C), want.stats[idx])
    assert np.array_equal(features_np.compute_row_features(C)[:, :13], want.feat32[idx])
    assert np.array_equal(features_np.topk_smallest(C).astype(np.float32), want.topk32[idx])
