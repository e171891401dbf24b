"""The synthetic cost families made on the MI355X (csrc/cost_families.hip) against the NumPy restatement of
cost_families_common.py: the draws, the seven families to the bit at the sizes around both tile dimensions, a mixed
batch in both layouts, independence of batch and layout, the training batches end to end, and the stream."""
import ctypes as ct

import numpy as np
import pytest

import cost_families_common as cf
from host_common import bits_equal, device_lib as lib, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def device_draws(lib, torch, seed, stream, kind, first, count, m=1, tail=3):
    """`count` draws and `tail` sentinel words after them."""
    dtype = torch.int32 if kind == 2 else torch.float64
    out = torch.full((count + tail,), -7, dtype=dtype, device="cuda:0")
    rc = lib.lapwarm_cost_family_draws(seed, stream, kind, first, count, m, out.data_ptr(), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[count:] == -7).all(), "wrote past the count"
    return got[:count]


def device_normals(lib, torch, seed):
    return lambda stream, count: device_draws(lib, torch, seed, stream, 1, 0, count)


def generate_raw(lib, torch, plan, padded, width=None):
    """lapwarm_generate_costs_ragged itself on [(family, n, seed, p0, p1)] (family a name or an id; n may be 0): the
    buffer pre-filled with SENTINEL, 5 words longer than the batch; returns (buffer, offsets, ret, ld)."""
    B = len(plan)
    sizes = [p[1] for p in plan]
    N = width or max(sizes)
    if padded:
        ld, offsets = N, [b * N * N for b in range(B)]
        total = B * N * N
    else:
        ld, offsets = 0, np.concatenate(([0], np.cumsum(np.asarray(sizes, dtype=np.int64) ** 2)))[:-1].tolist()
        total = int(sum(n * n for n in sizes))
    dev = "cuda:0"
    C = torch.full((total + 5,), SENTINEL, dtype=torch.float64, device=dev)
    fam = torch.tensor([cf.FAMILY_IDS.get(p[0], p[0]) for p in plan], dtype=torch.int32, device=dev)
    seeds = torch.from_numpy(np.asarray([p[2] for p in plan], dtype=np.uint64).view(np.int64)).to(dev)
    params = torch.tensor([[float(p[3]), float(p[4]), 0.0, 0.0] for p in plan], dtype=torch.float64, device=dev)
    offs = torch.tensor(offsets, dtype=torch.int64, device=dev)
    sz = torch.tensor(sizes, dtype=torch.int32, device=dev)
    ret = torch.full((B,), -1, dtype=torch.int32, device=dev)
    ws_bytes = lib.lapwarm_cost_families_workspace_bytes(B, N)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    rc = lib.lapwarm_generate_costs_ragged(C.data_ptr(), offs.data_ptr(), sz.data_ptr(), ld, B, N, fam.data_ptr(),
                                           seeds.data_ptr(), params.data_ptr(), ret.data_ptr(), ws.data_ptr(),
                                           ct.c_size_t(ws_bytes), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return C.cpu().numpy(), offsets, ret.cpu().tolist(), ld


def prefix(buf, offset, n, ld):
    stride = ld or n
    return np.stack([buf[offset + i * stride: offset + i * stride + n] for i in range(n)]) if n else np.zeros((0, 0))


def untouched_outside(buf, offsets, sizes, ld):
    """Every word that belongs to no prefix still holds the sentinel."""
    owned = np.zeros(buf.shape, dtype=bool)
    for o, n in zip(offsets, sizes):
        stride = ld or n
        for i in range(n):
            owned[o + i * stride: o + i * stride + n] = True
    return (buf[~owned] == SENTINEL).all() and not (buf[owned] == SENTINEL).any()


def test_uniform_and_integer_draws_are_the_restatement_to_the_bit(lib, torch_cuda):
    seed, first, count = cf.SEED_DRAWS, cf.DRAWS_FIRST, cf.DRAWS_COUNT
    assert seed >> 63 == 1 and first > 2**34 and count % 4
    for stream in (0, 4):
        got = device_draws(lib, torch_cuda, seed, stream, 0, first, count)
        assert bits_equal(got, cf.uniforms(seed, stream, first, count)), stream
    for m in (1, 5, 129, 2**31 - 1):
        got = device_draws(lib, torch_cuda, seed, 5, 2, first, count, m)
        assert np.array_equal(got.astype(np.int64), cf.integers(seed, 5, first, count, m)), m


def test_normal_draws_are_within_1e_14_of_the_wide_reference(lib, torch_cuda):
    """Z = r cos(t) or r sin(t) with r = sqrt(-2 log(1 - u1)), t = 6.283185307179586 u2, against the same formula
    carried in np.longdouble and rounded to double once.  The bound 1e-14 is derived, not measured.  1 - u1 is exact
    (u1 is a multiple of 2^-53 in [0, 1)) and at least 2^-53, so L = -2 log(1 - u1) <= 2 * 53 ln 2 = 73.5 and
    |Z| <= r <= sqrt(73.5) = 8.57.  With the accuracy the HIP math API documents for fp64 (log 1 ulp, sin, cos and
    sincos 2 ulp) and a correctly rounded sqrt, in absolute terms:
      trig:    2 ulp of a value below 1 is 2 * 2^-53 = 2.2e-16; times r:                                   1.90e-15
      t:       rounded once, t < 8, so off by at most 2^-51 = 4.4e-16, which moves sin and cos by at most
               as much; times r:                                                                           3.81e-15
      log:     1 ulp of L is at most 2^-52 relative, half of that in r = sqrt(L), plus the rounding of
               sqrt, 2^-53: r is off by 2^-52 relative, Z by 8.57 * 2.2e-16:                              1.90e-15
      product: one rounding, half an ulp of a value below 16:                                              0.89e-15
    which sum to 8.5e-15.  The reference carries a 64-bit significand (its own error is below 1e-17) and its one
    rounding to double adds another 0.89e-15: 9.4e-15 < 1e-14.  (Counting the rounding of t, which a sum of 7e-15
    leaves out, the terms still stay below the bound.)"""
    seed, first, count = cf.SEED_DRAWS, cf.DRAWS_FIRST, cf.DRAWS_COUNT
    worst = 0.0
    for stream in (1, 2):
        got = device_draws(lib, torch_cuda, seed, stream, 1, first, count)
        want = cf.normals_reference(seed, stream, first, count)
        err = float(np.abs(got - want).max())
        print(f"stream {stream}: max |Z - Z_ref| = {err:.3e}")
        worst = max(worst, err)
    assert worst <= 1e-14, worst


@pytest.fixture(scope="module")
def all_cases(lib, torch_cuda):
    """Every case of cost_families_common.cases() in one packed call: (plan, buffer, offsets, ret)."""
    plan = cf.cases()
    buf, offsets, ret, ld = generate_raw(lib, torch_cuda, plan, padded=False)
    return plan, buf, offsets, ret


def test_every_family_is_the_restatement_to_the_bit_around_both_tile_sizes(lib, torch_cuda, all_cases):
    plan, buf, offsets, ret = all_cases
    assert ret == [0] * len(plan)
    sizes = [p[1] for p in plan]
    assert {cf.TILE_ROWS + d for d in (-1, 0, 1)} | {cf.TILE_COLS + d for d in (-1, 0, 1)} | {1, 2, 3, 7} <= set(sizes)
    assert untouched_outside(buf, offsets, sizes, 0)
    for (family, n, seed, p0, p1), o in zip(plan, offsets):
        want = cf.matrix(family, n, seed, p0, p1, normals=device_normals(lib, torch_cuda, seed))
        got = prefix(buf, o, n, 0)
        assert bits_equal(got, want), (family, n, seed, p0, float(np.abs(got - want).max()))


def test_mixed_batch_packed_and_padded_with_an_empty_instance(lib, torch_cuda):
    plan = [(f, n, s, *cf.DEFAULTS[f]) for f, n, s in cf.MIXED]
    sizes = [p[1] for p in plan]
    want = [cf.matrix(f, n, s, p0, p1, normals=device_normals(lib, torch_cuda, s)) if n else None
            for f, n, s, p0, p1 in plan]
    for padded in (False, True):
        buf, offsets, ret, ld = generate_raw(lib, torch_cuda, plan, padded)
        assert ret == [0 if n else 2 for n in sizes], (padded, ret)
        assert untouched_outside(buf, offsets, sizes, ld), padded
        for b, n in enumerate(sizes):
            if n:
                assert bits_equal(prefix(buf, offsets[b], n, ld), want[b]), (padded, plan[b])
    # an instance is its own (family, n, seed, parameters): the same bits alone, packed
    from gnn import synthetic_pack
    for b, (f, n, s, p0, p1) in enumerate(plan):
        if n:
            alone = synthetic_pack([f], [n], [s]).C.cpu().numpy().reshape(n, n)
            assert bits_equal(alone, want[b]), plan[b]


def test_a_bad_family_or_rank_is_reported_on_the_device_and_not_written(lib, torch_cuda):
    plan = [("uniform", 5, 1, 0, 0.0), (7, 5, 2, 0, 0.0), (-1, 3, 3, 0, 0.0), ("low_rank", 4, 4, 65, 0.1),
            ("noisy_linear", 4, 5, 0, 0.1), ("tie", 6, 6, 5, 1e-6)]
    for padded in (False, True):
        buf, offsets, ret, ld = generate_raw(lib, torch_cuda, plan, padded)
        assert ret == [0, 3, 3, 3, 3, 0]
        live = [n if r == 0 else 0 for (_, n, *_), r in zip(plan, ret)]
        assert untouched_outside(buf, offsets, live, ld)
        assert bits_equal(prefix(buf, offsets[0], 5, ld), cf.matrix("uniform", 5, 1))
        assert bits_equal(prefix(buf, offsets[5], 6, ld), cf.matrix("tie", 6, 6))
    # a size above the padded width, or wider than the row stride: ret 2, no work
    buf, offsets, ret, ld = generate_raw(lib, torch_cuda, [("uniform", 9, 1, 0, 0.0), ("metric", 4, 2, 0, 0.0)], True,
                                         width=8)
    assert ret == [2, 0] and untouched_outside(buf, offsets, [0, 4], ld)


def test_synthetic_pack_layouts_and_the_numpy_convenience(lib, torch_cuda):
    from gnn import ragged_pack, synthetic_pack
    from solvers.generators import generate_family_device
    fams, sizes, seeds = ["sparse", "block", "metric", "tie"], [7, 9, 3, 8], [4, 2**64 - 1, 17, 2**63]
    params = [None, {"blocks": 2, "noise": 0.2}, None, {"bins": 3}]
    packed = synthetic_pack(fams, sizes, seeds, params=params)
    padded = synthetic_pack(fams, sizes, seeds, params=params, padded=True)
    assert packed.ld == 0 and padded.ld == 9 == packed.N == padded.N and tuple(padded.C.shape) == (4, 9, 9)
    assert packed.host_sizes == sizes and packed.sizes.tolist() == sizes
    mats = []
    for b, n in enumerate(sizes):
        o = int(packed.offsets[b])
        mats.append(packed.C[o:o + n * n].reshape(n, n).cpu().numpy())
        assert bits_equal(padded.C[b, :n, :n].cpu().numpy(), mats[b])
        assert float(padded.C[b, n:, :].abs().sum()) == 0.0 and float(padded.C[b, :, n:].abs().sum()) == 0.0
    assert bits_equal(mats[0], cf.matrix("sparse", 7, 4))
    assert bits_equal(mats[2], cf.matrix("metric", 3, 17))
    assert bits_equal(mats[3], cf.matrix("tie", 8, 2**63, 3, 1e-6))
    assert bits_equal(mats[1], cf.matrix("clustered", 9, 2**64 - 1, 2, 0.2,
                                         normals=device_normals(lib, torch_cuda, 2**64 - 1)))
    same = ragged_pack(mats, "cuda:0")  # the pack the parent's route gives for those matrices
    assert torch_cuda.equal(same.C, packed.C) and torch_cuda.equal(same.offsets, packed.offsets)
    assert bits_equal(generate_family_device("block", 9, 2**64 - 1, blocks=2, noise=0.2), mats[1])
    assert bits_equal(generate_family_device("sparse", 7, 4), mats[0])


E2E = (["uniform", "sparse", "metric", "clustered"], [5, 33, 70, 64], [11, 12, 13, 14])


def equal_fields(torch, got, want, names):
    for name in names:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name


def test_synthetic_training_batch_is_training_batch_of_the_downloaded_matrices(torch_cuda):
    torch = torch_cuda
    from gnn import OneGNN, WarmStartPipeline, synthetic_pack
    torch.manual_seed(0)
    pipe = WarmStartPipeline(OneGNN(21, hidden=32, layers=1).eval(), torch.device("cuda:0"))
    pack = synthetic_pack(*E2E)
    mats = [pack.C[int(o):int(o) + n * n].reshape(n, n).cpu().numpy() for o, n in zip(pack.offsets, E2E[1])]
    names = ("cost", "u", "v", "row_feat", "topk", "mask", "sizes")
    equal_fields(torch, pipe.synthetic_training_batch(*E2E), pipe.training_batch(mats), names)
    g1, g2 = (torch.Generator(device="cuda:0").manual_seed(5) for _ in range(2))
    noisy = pipe.synthetic_training_batch(*E2E, dual_noise_std=0.15, dual_noise_prob=1.0, generator=g1)
    want = pipe.training_batch(mats, dual_noise_std=0.15, dual_noise_prob=1.0, generator=g2)
    equal_fields(torch, noisy, want, names)
    assert not torch.equal(noisy.u, pipe.training_batch(mats).u)


def test_synthetic_dual_training_batch_is_dual_training_batch_of_the_downloaded_matrices(torch_cuda):
    torch = torch_cuda
    from gnn import synthetic_pack
    from gnn.dual_gnn import DualGNN
    from gnn.pipeline import DualWarmStartPipeline
    torch.manual_seed(0)
    pipe = DualWarmStartPipeline(DualGNN(hidden_dim=16, layers=2, heads=4).eval(), torch.device("cuda:0"))
    pack = synthetic_pack(*E2E)
    mats = [pack.C[int(o):int(o) + n * n].reshape(n, n).cpu().numpy() for o, n in zip(pack.offsets, E2E[1])]
    names = ("cost", "u", "v", "row_feat", "col_feat", "edge_feat", "mask", "sizes")
    equal_fields(torch, pipe.synthetic_dual_training_batch(*E2E), pipe.dual_training_batch(mats), names)
    g1, g2 = (torch.Generator(device="cuda:0").manual_seed(5) for _ in range(2))
    noisy = pipe.synthetic_dual_training_batch(*E2E, dual_noise_std=0.15, dual_noise_prob=1.0, generator=g1)
    want = pipe.dual_training_batch(mats, dual_noise_std=0.15, dual_noise_prob=1.0, generator=g2)
    equal_fields(torch, noisy, want, names)


def test_stream_packs_follow_the_plans_and_differ_from_one_another(torch_cuda):
    from gnn import SyntheticStream, synthetic_pack
    fams, sizes = ("uniform", "sparse", "metric", "clustered"), (5, 9, 33)
    plans = SyntheticStream(fams, sizes, 4, 3)
    packs = SyntheticStream(fams, sizes, 4, 3).packs("cuda:0")
    first, second = next(packs), next(packs)
    p1, p2 = next(plans), next(plans)
    assert first.host_sizes == p1[1] and second.host_sizes == p2[1]
    assert torch_cuda.equal(first.C, synthetic_pack(*p1).C) and torch_cuda.equal(second.C, synthetic_pack(*p2).C)
    assert first.C.shape != second.C.shape or not torch_cuda.equal(first.C, second.C)
