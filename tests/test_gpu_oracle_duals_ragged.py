"""Oracle duals of mixed-size batches on the MI355X: one lapwarm_oracle_duals_ragged call against the golden
vectors of the reference and against the uniform call on every instance alone, bit for bit, in both pack forms;
the per-instance sweep budget inside the shared chunk schedule; failing and malformed instances beside good ones;
and the public path up to a labelled DeviceBatch."""
import ctypes as ct

import numpy as np
import pytest

from host_common import bits_equal, small_model_pipe as pipe  # noqa: F401
from oracle_duals_common import OracleCases, jacobi, make_C, oracle_from_v
from oracle_duals_ragged_common import EMPTY, chain_instance

pytestmark = pytest.mark.gpu

CASES = OracleCases()
DIFF = CASES.indices("diff")
SIZES = (1, 2, 3, 7, 8, 33, 64, 129, 255, 256, 257, 511, 513, 640)
FAMILIES = ("uniform", "sparse", "tie", "metric", "int100")


def alone(pipe, C, x):
    """oracle_duals_batch of one instance: u, v, ret, sweeps on the host."""
    import torch
    Cd = torch.from_numpy(np.ascontiguousarray(C)).to("cuda:0").unsqueeze(0)
    xd = torch.from_numpy(np.asarray(x, dtype=np.int32)).to("cuda:0").unsqueeze(0)
    _, u, v, ret, sweeps = pipe.oracle_duals_batch(Cd, xd)
    return u[0].cpu().numpy(), v[0].cpu().numpy(), int(ret[0]), sweeps[0].cpu().numpy()


def alone_pairs(pipe, C, rows, cols):
    """lapwarm_oracle_duals_batched of one instance with its pairs in the caller's order."""
    import torch
    n = C.shape[0]
    dev = "cuda:0"
    Cd = torch.from_numpy(np.ascontiguousarray(C)).to(dev)
    r = torch.from_numpy(np.asarray(rows, dtype=np.int32)).to(dev)
    c = torch.from_numpy(np.asarray(cols, dtype=np.int32)).to(dev)
    u, v = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    ret, sweeps = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
    nbytes = pipe.lib.lapwarm_oracle_duals_workspace_bytes(1, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = pipe.lib.lapwarm_oracle_duals_batched(Cd.data_ptr(), 1, n, r.data_ptr(), c.data_ptr(), u.data_ptr(),
                                               v.data_ptr(), ret.data_ptr(), sweeps.data_ptr(), ws.data_ptr(), nbytes,
                                               ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return u.cpu().numpy(), v.cpu().numpy(), int(ret[0]), sweeps.cpu().numpy()


def ragged_abi(pipe, pack, rows, cols, sizes_dev=None, host_sizes=None):
    """lapwarm_oracle_duals_ragged through the C ABI: rows, cols (B, N) int32 on the host; `sizes_dev` replaces
    the sizes the device reads, `host_sizes` the host's copy.  Everything comes back on the host."""
    import torch
    B, N, dev = len(pack.host_sizes), pack.N, pack.C.device
    r = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(cols, dtype=np.int32)).to(dev)
    sizes = pack.sizes if sizes_dev is None else torch.tensor(sizes_dev, dtype=torch.int32, device=dev)
    u = torch.full((B, N), 7.0, dtype=torch.float64, device=dev)
    v = torch.full((B, N), 7.0, dtype=torch.float64, device=dev)
    ret = torch.full((B,), -9, dtype=torch.int32, device=dev)
    sweeps = torch.full((B, 4), -9, dtype=torch.int32, device=dev)
    nbytes = pipe.lib.lapwarm_oracle_duals_ragged_workspace_bytes(B, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = pipe.lib.lapwarm_oracle_duals_ragged(
        pack.C.data_ptr(), pack.offsets.data_ptr(), sizes.data_ptr(), (ct.c_int * B)(*(host_sizes or pack.host_sizes)), pack.ld, B,
        N, r.data_ptr(), c.data_ptr(), u.data_ptr(), v.data_ptr(), ret.data_ptr(), sweeps.data_ptr(), ws.data_ptr(),
        nbytes, ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return u.cpu().numpy(), v.cpu().numpy(), ret.cpu().numpy(), sweeps.cpu().numpy()


def padded_rows_cols(pairs, N):
    rows = np.full((len(pairs), N), -1, dtype=np.int32)
    cols = np.full((len(pairs), N), -1, dtype=np.int32)
    for b, (r, c) in enumerate(pairs):
        rows[b, :len(r)], cols[b, :len(c)] = r, c
    return rows, cols


def ragged(pipe, mats, xs, padded=False):
    """oracle_duals_ragged of the instances, packed or as a padded (B, N, N) block with sizes -> host arrays."""
    import torch

    from gnn.features import ragged_pack
    sizes = [m.shape[0] for m in mats]
    N = max(sizes)
    if padded:
        block = np.full((len(mats), N, N), np.nan)  # nothing outside a prefix may be read into a result
        for b, m in enumerate(mats):
            block[b, :m.shape[0], :m.shape[0]] = m
        pack = ragged_pack(block, "cuda:0", sizes=sizes)
    else:
        pack = ragged_pack(mats, "cuda:0")
    X = np.full((len(mats), N), -7, dtype=np.int64)
    for b, x in enumerate(xs):
        X[b, :len(x)] = x
    u, v, ret, sweeps = pipe.oracle_duals_ragged(pack, torch.from_numpy(X).to("cuda:0"))
    torch.cuda.synchronize()
    return u.cpu().numpy(), v.cpu().numpy(), ret.cpu().numpy(), sweeps.cpu().numpy()


def assert_equal_to_alone(got, b, n, ref, what):
    u, v, ret, sweeps = got
    ua, va, ra, sa = ref
    assert int(ret[b]) == ra, (what, int(ret[b]), ra)
    assert np.array_equal(sweeps[b], sa), (what, sweeps[b], sa)
    assert bits_equal(u[b, :n], ua) and bits_equal(v[b, :n], va), what  # (NaN payloads included)
    assert not u[b, n:].any() and not v[b, n:].any(), what  # 0 beyond the prefix


# ---- 1. golden ----

def test_all_golden_cases_in_one_ragged_call(pipe):
    from gnn.features import ragged_pack
    cases = [CASES.case(k) for k in DIFF]
    assert len(cases) == 38 and min(m["n"] for m in cases) == 1 and max(m["n"] for m in cases) == 1024
    pack = ragged_pack([m["C"] for m in cases], "cuda:0")
    rows, cols = padded_rows_cols([(m["rows"], m["cols"]) for m in cases], pack.N)
    u, v, ret, sweeps = ragged_abi(pipe, pack, rows, cols)
    seen = set()
    for b, m in enumerate(cases):
        n = m["n"]
        seen.add(m["outcome"])
        if m["outcome"] == "ok":
            assert ret[b] == 0, (m["label"], ret[b])
            assert bits_equal(u[b, :n], m["u"]) and bits_equal(v[b, :n], m["v"]), m["label"]
        elif m["outcome"] == "RuntimeError":
            assert ret[b] == 1, (m["label"], ret[b])
        else:
            assert m["outcome"] == "AssertionError"
            ua, va, ra, sa = alone_pairs(pipe, m["C"], m["rows"], m["cols"])
            assert ra in (2, 3) and ret[b] == ra, (m["label"], ret[b], ra)
            assert bits_equal(u[b, :n], ua) and bits_equal(v[b, :n], va) and np.array_equal(sweeps[b], sa)
        if ret[b] == 1:
            assert np.isnan(u[b, :n]).all() and np.isnan(v[b, :n]).all(), m["label"]
        assert not u[b, n:].any() and not v[b, n:].any(), m["label"]
    assert seen == {"ok", "RuntimeError", "AssertionError"}


# ---- 2. equal to alone, both pack forms ----

@pytest.fixture(scope="module")
def family_batch(pipe):
    """Every size in every family, its lap.lapjv matching and the uniform call on it alone: computed once."""
    import lap
    mats, xs, refs, labels = [], [], [], []
    for fam in FAMILIES:
        for n in SIZES:
            C = make_C((fam, n, 5))
            _, x, _ = lap.lapjv(C)
            mats.append(C)
            xs.append(np.asarray(x))
            refs.append(alone(pipe, C, x))
            labels.append(f"{fam}_n{n}")
    return mats, xs, refs, labels


@pytest.mark.parametrize("padded", (False, True), ids=("packed", "padded"))
def test_every_instance_equals_the_uniform_call_alone(pipe, family_batch, padded):
    mats, xs, refs, labels = family_batch
    if not padded:  # odd offsets occur, so both load paths run
        off = np.cumsum([0] + [m.size for m in mats[:-1]])
        assert (off % 2 == 1).any() and (off % 2 == 0).any()
    got = ragged(pipe, mats, xs, padded)
    for b, (m, ref, label) in enumerate(zip(mats, refs, labels)):
        assert_equal_to_alone(got, b, m.shape[0], ref, label)
    # (the smallest sizes are the reference's negative cycle: its single round updates and the tol check fires)
    assert all(r[2] == 0 for m, r in zip(mats, refs) if m.shape[0] >= 33), [l for l, r in zip(labels, refs) if r[2]]


# ---- 3. a budget that ends inside a shared chunk ----

@pytest.mark.parametrize("chains_first", (True, False), ids=("chains_first", "chains_last"))
def test_chain_instances_keep_their_own_budget(pipe, chains_first):
    import lap
    chains = [chain_instance(n) for n in (7, 13, 37)]
    for C in chains:
        n = C.shape[0]
        i = np.arange(n)
        vj, sj = jacobi(C, i, i)
        assert sj == n  # one sweep more than the budget n - 1
        uj, vj = oracle_from_v(C, i, i, vj)
        assert ((C - uj[:, None]) - vj[None, :]).min() == 0.0
    U = make_C(("uniform", 300, 9))
    _, xu, _ = lap.lapjv(U)
    mats = chains + [U] if chains_first else [U] + chains
    xs = [np.arange(m.shape[0]) if m is not U else np.asarray(xu) for m in mats]
    got = ragged(pipe, mats, xs)
    for b, (m, x) in enumerate(zip(mats, xs)):
        ref = alone(pipe, m, x)
        assert_equal_to_alone(got, b, m.shape[0], ref, (chains_first, m.shape[0]))
        if m is not U:
            assert got[2][b] == 0 and got[3][b, 3] == 1 and got[3][b, 0] == m.shape[0] - 1, got[3][b]
        else:
            assert got[2][b] == 0 and got[3][b, 3] == 0


# ---- 4. non-optimal matchings ----

def test_non_optimal_matchings_fail_alone(pipe):
    import lap
    sizes = (8, 512, 2049, 96)
    mats = [make_C(("uniform", n, 21)) for n in sizes]
    xs = [np.asarray(lap.lapjv(C)[1]) for C in mats]
    good = [alone(pipe, C, x) for C, x in zip(mats, xs)]
    xs[1], xs[2] = np.roll(xs[1], 1), np.roll(xs[2], 1)
    u, v, ret, sweeps = got = ragged(pipe, mats, xs)
    assert ret[1] == 1 and ret[2] == 1
    assert sweeps[1, 3] == 1 and sweeps[2, 3] == 0  # 512 is replayed, 2049 is above the replay's limit
    for b in (1, 2):
        assert np.isnan(u[b, :sizes[b]]).all() and np.isnan(v[b, :sizes[b]]).all()
        assert not u[b, sizes[b]:].any() and not v[b, sizes[b]:].any()
    for b in (0, 3):
        assert good[b][2] == 0
        assert_equal_to_alone(got, b, sizes[b], good[b], sizes[b])


# ---- 5. bad input ----

def test_bad_instances_get_their_codes_and_leave_the_neighbours_alone(pipe):
    import lap

    from gnn.features import ragged_pack
    sizes = (33, 20, 64, 17, 50)
    mats = [make_C(("uniform", n, 4)) for n in sizes]
    xs = [np.asarray(lap.lapjv(C)[1]) for C in mats]
    good = [alone(pipe, C, x) for C, x in zip(mats, xs)]
    bad_x = list(xs)
    bad_x[1] = xs[1].copy()
    bad_x[1][3] = bad_x[1][4]  # not a permutation
    bad_mats = [m.copy() for m in mats]
    bad_mats[2][5, 9] = np.nan
    bad_mats[3][0, 16] = np.inf
    u, v, ret, sweeps = got = ragged(pipe, bad_mats, bad_x)
    assert list(ret) == [0, 4, 5, 5, 0]
    for b in (0, 4):
        assert_equal_to_alone(got, b, sizes[b], good[b], sizes[b])
    for b in (1, 2, 3):
        assert np.isnan(u[b, :sizes[b]]).all() and not u[b, sizes[b]:].any()

    # sizes the device treats as empty: 0, and one above N
    pack = ragged_pack(mats, "cuda:0")
    rows, cols = padded_rows_cols([(np.arange(n), x) for n, x in zip(sizes, xs)], pack.N)
    dev_sizes = [33, 0, 64, pack.N + 1, 50]
    u, v, ret, sweeps = got = ragged_abi(pipe, pack, rows, cols, dev_sizes)
    assert list(ret) == [0, EMPTY, 0, EMPTY, 0]
    for b in (0, 2, 4):
        assert_equal_to_alone(got, b, sizes[b], good[b], sizes[b])
    for b in (1, 3):
        assert not u[b].any() and not v[b].any() and not sweeps[b].any()


def test_a_size_wider_than_the_row_stride_is_empty(pipe):
    """The third empty condition: 1 <= n_b <= N but n_b > ld > 0.  Blocks of 40 x 40 with row stride 40 under a
    padded width of 48; the middle instance claims 44."""
    import lap
    import torch

    from gnn.features import RaggedPack
    ld, N, sizes = 40, 48, (33, 44, 40)
    mats = [make_C(("uniform", min(n, ld), 6)) for n in sizes]
    xs = [np.asarray(lap.lapjv(C)[1]) for C in mats]
    block = np.full((3, ld, ld), np.nan)
    for b, m in enumerate(mats):
        block[b, :m.shape[0], :m.shape[0]] = m
    dev = torch.device("cuda:0")
    pack = RaggedPack(torch.from_numpy(block).to(dev), torch.arange(3, device=dev) * (ld * ld),
                      torch.tensor(sizes, dtype=torch.int32, device=dev), None, None, ld, N, list(sizes))
    rows, cols = padded_rows_cols([(np.arange(len(x)), x) for x in xs], N)
    u, v, ret, sweeps = got = ragged_abi(pipe, pack, rows, cols)
    assert list(ret) == [0, EMPTY, 0]
    assert not u[1].any() and not v[1].any() and not sweeps[1].any()
    for b in (0, 2):
        assert_equal_to_alone(got, b, sizes[b], alone(pipe, mats[b], xs[b]), sizes[b])


def test_a_device_size_above_every_host_size_never_reports_ok_without_duals(pipe):
    """The host's budget ends the schedule before the chain instance's own: the last check hands it to the
    replay, which is exact, so u and v are the instance's own and `replayed` is set; ret is not 0 beside NaN."""
    import lap

    from gnn.features import ragged_pack
    chain, U = chain_instance(37), make_C(("uniform", 20, 2))
    xu = np.asarray(lap.lapjv(U)[1])
    pack = ragged_pack([chain, U], "cuda:0")
    rows, cols = padded_rows_cols([(np.arange(37), np.arange(37)), (np.arange(20), xu)], pack.N)
    u, v, ret, sweeps = got = ragged_abi(pipe, pack, rows, cols, host_sizes=[10, 20])
    ua, va, ra, sa = alone(pipe, chain, np.arange(37))
    assert ra == 0 and ret[0] == 0 and sweeps[0, 3] == 1 and sweeps[0, 0] == 19, (ret, sweeps)
    assert bits_equal(u[0, :37], ua) and bits_equal(v[0, :37], va)
    assert_equal_to_alone(got, 1, 20, alone(pipe, U, xu), "uniform beside it")


def test_python_layer_raises_value_error_before_device_work(pipe):
    import torch

    from gnn.features import RaggedPack, ragged_pack
    mats = [make_C(("uniform", n, 4)) for n in (5, 9)]
    pack = ragged_pack(mats, "cuda:0")
    x = torch.zeros((2, 9), dtype=torch.int64, device="cuda:0")
    with pytest.raises(ValueError):  # float32 costs
        pipe.oracle_duals_many([torch.from_numpy(m.astype(np.float32)).to("cuda:0") for m in mats])
    p32 = RaggedPack(pack.C.to(torch.float32), pack.offsets, pack.sizes, pack.pos_off, pack.posenc, pack.ld, pack.N,
                     pack.host_sizes)
    with pytest.raises(ValueError):
        pipe.oracle_duals_ragged(p32, x)
    for bad in (x[:, :8], x[:1], x.reshape(-1), x.to(torch.float64), x.cpu()):
        with pytest.raises(ValueError):
            pipe.oracle_duals_ragged(pack, bad)
    with pytest.raises(ValueError):
        pipe.oracle_duals_many(mats, x=[np.arange(5)])


# ---- 6. the public path ----

def test_training_batch_is_collate_device_with_device_labels(pipe):
    import torch

    from gnn import collate_device
    from gnn.losses import warmstart_loss
    from solvers import compute_oracle_duals
    sizes = (48, 64, 100, 129)
    mats = [make_C(("uniform", n, 13)) for n in sizes]
    items = []
    for C in mats:
        u, v = compute_oracle_duals(C)
        items.append({"cost": C, "u": u, "v": v})
    want = collate_device(items, "cuda:0")
    got = pipe.training_batch(mats)
    torch.cuda.synchronize()
    for name in ("mask", "row_feat", "topk", "cost", "sizes", "u", "v"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    u_pred = torch.zeros_like(got.u, requires_grad=True)
    loss = warmstart_loss(got.cost, u_pred, got.u, got.mask)
    loss = loss[0] if isinstance(loss, (tuple, list)) else loss
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(u_pred.grad).all()


def test_oracle_duals_many_takes_its_matching_from_the_seeded_solve(pipe):
    import lap
    import torch
    sizes = (48, 64, 100, 129)
    mats = [make_C(("uniform", n, 13)) for n in sizes]
    out = pipe.oracle_duals_many(mats)
    torch.cuda.synchronize()
    for C, (x, u, v, ret, sweeps) in zip(mats, out):
        _, xl, _ = lap.lapjv(C)
        assert np.array_equal(x.cpu().numpy(), xl)
        ua, va, ra, sa = alone(pipe, C, xl)
        assert int(ret) == 0 == ra and np.array_equal(sweeps.cpu().numpy(), sa)
        assert bits_equal(u.cpu().numpy(), ua) and bits_equal(v.cpu().numpy(), va)


def test_oracle_duals_many_reads_a_stacked_block_and_a_padded_matching_in_place(pipe):
    import lap
    import torch
    mats = [make_C(("uniform", 64, s)) for s in (1, 2, 3)]
    xs = np.stack([np.asarray(lap.lapjv(C)[1]) for C in mats]).astype(np.int32)
    block = torch.from_numpy(np.stack(mats)).to("cuda:0")
    out = pipe.oracle_duals_many(block, torch.from_numpy(xs).to("cuda:0"))
    lists = pipe.oracle_duals_many(mats, [x for x in xs])
    torch.cuda.synchronize()
    for C, x, (xo, u, v, ret, sweeps), (xl, ul, vl, rl, sl) in zip(mats, xs, out, lists):
        ua, va, ra, sa = alone(pipe, C, x)
        assert xo.dtype == torch.int32 and np.array_equal(xo.cpu().numpy(), x) and int(ret) == ra == int(rl) == 0
        assert bits_equal(u.cpu().numpy(), ua) and bits_equal(v.cpu().numpy(), va)
        assert bits_equal(ul.cpu().numpy(), ua) and bits_equal(vl.cpu().numpy(), va)
        assert np.array_equal(sweeps.cpu().numpy(), sa) and np.array_equal(sl.cpu().numpy(), sa)
    # matchings as tensors on the device: padded there, in their own integer type
    dev_list = pipe.oracle_duals_many(mats, [torch.from_numpy(x).to("cuda:0") for x in xs])
    assert len(dev_list) == 3 and dev_list.x.dtype == torch.int32 and tuple(dev_list.u.shape) == (3, 64)
    for (xo, u, v, ret, sweeps), (xd, ud, vd, rd, sd) in zip(out, dev_list[0:3]):
        assert torch.equal(xo, xd) and torch.equal(u, ud) and torch.equal(v, vd) and torch.equal(sweeps, sd)
    with pytest.raises(ValueError):
        pipe.oracle_duals_many(block, torch.from_numpy(xs[:2]).to("cuda:0"))
    with pytest.raises(ValueError):
        pipe.oracle_duals_many(block, torch.from_numpy(xs))  # a padded matching on another device


def test_training_batch_names_the_instance_that_fails(pipe):
    C = np.full((1, 1), 3.0)  # n = 1 is the reference's negative cycle
    with pytest.raises(RuntimeError, match=r"instance 1 .*code 1"):
        pipe.training_batch([make_C(("uniform", 12, 1)), C])
