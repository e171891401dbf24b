"""Relax steps with several tie events on the MI355X: the finders of a step rank their events from the event bitmap
and swap their own columns; a free column among the events ends the path; an event inside the swap window goes to the
ordered replay.  Integer costs from {0..3} and {0..7} make such steps the rule.  Expected (ret, x, y) and the control
flow counters come from oracle.jv.seeded_raw, without any tolerance; tests/multi_event_common.py classifies the relax
steps of the inputs on the CPU, and the inputs must contain every class."""
import functools

import numpy as np
import pytest

import multi_event_common as mec
from multi_event_common import make_pack, padded_seeds

COUNTERS = ((4, "paths"), (5, "finds"), (6, "scan_steps"), (7, "scan_elems"), (11, "arr_iters"))


@functools.lru_cache(maxsize=None)
def pipe():
    import torch

    from gnn import OneGNN, WarmStartPipeline
    torch.manual_seed(0)
    return WarmStartPipeline(OneGNN(21, 64, 2).cuda().eval())


@functools.lru_cache(maxsize=None)
def expected(k):
    from oracle import jv
    return jv.seeded_raw(*mec.case(k))


def check(k, x, y, ret, stats):
    r, xo, yo, so = expected(k)
    assert r == 0 and int(ret) == 0, (mec.CASES[k], r, int(ret), int(stats[12]))
    assert np.array_equal(xo, x) and np.array_equal(yo, y), mec.CASES[k]
    for q, name in COUNTERS:
        assert stats[q] == so[name], (mec.CASES[k], name, stats[q], so[name])


def solve(k):
    import torch
    C, u, v = (torch.from_numpy(a).cuda()[None] for a in mec.case(k))
    x, y, ret, stats = pipe().seeded_batch(C, u, v)
    return x[0].cpu().numpy(), y[0].cpu().numpy(), ret[0].cpu().numpy(), stats[0].cpu().numpy()


def test_the_inputs_contain_every_class_of_step():
    """A test-design check, on the CPU: the hard-coded inputs together hold each class at least once, those of the
    sizes with two bitmap words per lane do so among themselves, and the classifier walks the solve the oracle
    walks (same paths, minima collections and relax steps)."""
    total, large = dict.fromkeys(mec.CLASSES, 0), dict.fromkeys(mec.CLASSES, 0)
    for k, c in enumerate(mec.CASES):
        if not mec.classified(c):
            continue
        counts, walked = mec.classify(*mec.case(k))
        so = expected(k)[3]
        assert walked == (so["paths"], so["finds"], so["scan_steps"]), (c, walked, so)
        for name in mec.CLASSES:
            total[name] += counts[name]
            if c[0] >= mec.TWO_WORDS_PER_LANE:
                large[name] += counts[name]
    print(total, large)
    assert all(total.values()), total
    assert all(large.values()), large


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(mec.CASES)), ids=lambda k: "n%d-c%d-%s-%d" % mec.CASES[k])
def test_seeded_solve_equals_the_oracle(k):
    check(k, *solve(k))


@pytest.mark.gpu
def test_three_sizes_in_one_ragged_call():
    ks = [next(k for k, c in enumerate(mec.CASES) if c[0] == n and c[1] == 7) for n in mec.RAGGED_SIZES]
    assert all(pipe().ragged_solve_eligible(n) for n in mec.RAGGED_SIZES)
    p = make_pack([mec.case(k)[0] for k in ks])
    u, v = padded_seeds([mec.case(k)[1:] for k in ks], p.N)
    x, y, ret, stats = (t.cpu().numpy() for t in pipe().seeded_ragged(p, u, v, 1e-12))
    for b, k in enumerate(ks):
        n = mec.CASES[k][0]
        check(k, x[b, :n], y[b, :n], ret[b], stats[b])
        assert (x[b, n:] == -1).all() and (y[b, n:] == -1).all(), n


@pytest.mark.gpu
@pytest.mark.parametrize("n", (65, 2048))
def test_poisoned_workspace(n):
    """Every word of the workspace 0xFF before the solve: an event bitmap word or a control word read before it is
    written would show."""
    import torch
    k = next(k for k, c in enumerate(mec.CASES) if c[0] == n)
    C, u, v = (torch.from_numpy(a).cuda()[None] for a in mec.case(k))
    pipe().seeded_batch(C, u, v)  # (allocates the workspace of this shape)
    torch.cuda.synchronize()
    with torch.inference_mode():
        pipe()._workspace(1, n)[0].fill_(0xFF)
    x, y, ret, stats = pipe().seeded_batch(C, u, v)
    check(k, x[0].cpu().numpy(), y[0].cpu().numpy(), ret[0].cpu().numpy(), stats[0].cpu().numpy())
