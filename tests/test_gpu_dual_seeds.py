"""The ragged dual utilities on the MI355X: lapwarm_rowmin_ragged, lapwarm_project_feasible_ragged and
lapwarm_reduce_costs_ragged (csrc/ragged_batch.hip) through ctypes, WarmStartPipeline, gnn.row_min_ragged and the
*_many functions of `solvers`.

Every value the kernels produce is a minimum or a difference of two doubles, so results are compared for
equality (np.array_equal, with NaN where the other has NaN: `same`), never within a tolerance: against the
reference's results in tests/golden/dual_seeds_cases.npz, and against the uniform entries at the sizes where
the sweeps change shape."""
import ctypes as ct
import functools
import re

import numpy as np
import pytest

from conftest import PKG
from dual_seeds_common import case_key, case_names, cases, combos, matrix, np_project, np_reduce, same
from host_common import padded, shared_pipe as pipe  # noqa: F401

pytestmark = pytest.mark.gpu

LAYOUTS = ("packed", "padded")


def pack(mats, layout):
    from gnn.features import ragged_pack
    if layout == "packed":
        p = ragged_pack(list(mats))
        assert p.ld == 0
        return p
    N = max(m.shape[0] for m in mats)
    p = ragged_pack(padded(mats, N), sizes=[m.shape[0] for m in mats])
    assert p.ld == N
    return p


def pad_vectors(vectors, N, fill=np.nan):
    """(B, N) with NaN beyond every prefix: the entries read the prefix only."""
    import torch
    out = np.full((len(vectors), N), fill)
    for b, x in enumerate(vectors):
        out[b, :len(x)] = x
    return torch.from_numpy(out).cuda()


def poisoned_ws(lib, B, N):
    import torch
    nbytes = int(lib.lapwarm_ragged_duals_workspace_bytes(B, N))
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda"), nbytes


def raw_project(p, us, vs, max_rounds, tol, sizes=None):
    """lapwarm_project_feasible_ragged through ctypes with a 0xFF workspace and gmin NaN, rounds and ret -1 before
    the call; `sizes` replaces the pack's device sizes.  Returns host arrays u, v (B, N), gmin, rounds, ret."""
    import torch

    from lap import _hip
    lib = _hip.require_device()
    B, N = len(p.host_sizes), p.N
    u, v = pad_vectors(us, N), pad_vectors(vs, N)
    gmin = torch.full((B,), np.nan, dtype=torch.float64, device="cuda")
    rounds = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ret = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ws, nbytes = poisoned_ws(lib, B, N)
    sz = p.sizes if sizes is None else torch.tensor(sizes, dtype=torch.int32, device="cuda")
    rc = lib.lapwarm_project_feasible_ragged(p.C.data_ptr(), p.offsets.data_ptr(), sz.data_ptr(), p.ld, B, N,
                                             u.data_ptr(), v.data_ptr(), max_rounds, tol, gmin.data_ptr(),
                                             rounds.data_ptr(), ret.data_ptr(), ws.data_ptr(), nbytes,
                                             ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, _hip.last_error())
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (u, v, gmin, rounds, ret))


def raw_reduce(p, us, vs, shift, want_matrix=True, sizes=None):
    """lapwarm_reduce_costs_ragged through ctypes into an `out` full of NaN, gmin NaN, ret -1, workspace 0xFF."""
    import torch

    from lap import _hip
    lib = _hip.require_device()
    B, N = len(p.host_sizes), p.N
    u, v = pad_vectors(us, N), pad_vectors(vs, N)
    out = torch.full_like(p.C, np.nan) if want_matrix else None
    gmin = torch.full((B,), np.nan, dtype=torch.float64, device="cuda")
    ret = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ws, nbytes = poisoned_ws(lib, B, N)
    sz = p.sizes if sizes is None else torch.tensor(sizes, dtype=torch.int32, device="cuda")
    rc = lib.lapwarm_reduce_costs_ragged(p.C.data_ptr(), p.offsets.data_ptr(), sz.data_ptr(), p.ld, B, N,
                                         u.data_ptr(), v.data_ptr(), int(shift),
                                         out.data_ptr() if want_matrix else None, gmin.data_ptr(), ret.data_ptr(),
                                         ws.data_ptr(), nbytes, ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, _hip.last_error())
    torch.cuda.synchronize()
    return (out.cpu().numpy().reshape(-1) if want_matrix else None), gmin.cpu().numpy(), ret.cpu().numpy()


def raw_rowmin(p, vs=None, sizes=None):
    import torch

    from lap import _hip
    lib = _hip.require_device()
    B, N = len(p.host_sizes), p.N
    v = pad_vectors(vs, N) if vs is not None else None
    out = torch.full((B, N), np.nan, dtype=torch.float64, device="cuda")
    ret = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ws, nbytes = poisoned_ws(lib, B, N)
    sz = p.sizes if sizes is None else torch.tensor(sizes, dtype=torch.int32, device="cuda")
    rc = lib.lapwarm_rowmin_ragged(p.C.data_ptr(), p.offsets.data_ptr(), sz.data_ptr(), p.ld, B, N,
                                   v.data_ptr() if v is not None else None, out.data_ptr(), ret.data_ptr(),
                                   ws.data_ptr(), nbytes, ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, _hip.last_error())
    torch.cuda.synchronize()
    return out.cpu().numpy(), ret.cpu().numpy()


def matrix_of(flat, p, b):
    """Instance b of a buffer in the layout of the pack's C."""
    n, off = p.host_sizes[b], int(p.offsets[b])
    return np.lib.stride_tricks.as_strided(flat[off:], shape=(n, n), strides=(8 * (p.ld or n), 8)).copy()


@functools.lru_cache(maxsize=None)
def fixture_batch():
    """Every case of the fixture as one batch: names, matrices, seeds."""
    z = cases()
    names = case_names()
    mats = tuple(matrix(kind, n) for kind, n, _ in names)
    us = tuple(z[f"u0__{case_key(*c)}"] for c in names)
    vs = tuple(z[f"v0__{case_key(*c)}"] for c in names)
    return names, mats, us, vs


# ------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("a,b,max_rounds,tol", combos())
def test_fixture_cases_of_one_max_rounds_and_tol_in_one_batch(layout, a, b, max_rounds, tol):
    z = cases()
    names, mats, us, vs = fixture_batch()
    p = pack(mats, layout)
    u, v, gmin, rounds, ret = raw_project(p, us, vs, max_rounds, tol)
    want_rounds = [int(z[f"rounds__{case_key(*c)}"][a, b]) for c in names]
    assert rounds.tolist() == want_rounds and (ret == 0).all()
    if max_rounds == 3 and tol < 0:
        assert len(set(want_rounds)) > 1  # instances of one call stop at different rounds
    for k, (c, r) in enumerate(zip(names, want_rounds)):
        key, n = f"{case_key(*c)}__r{r}", c[1]
        assert np.array_equal(u[k, :n], z[f"u__{key}"], equal_nan=True), key
        assert np.array_equal(v[k, :n], z[f"v__{key}"], equal_nan=True), key
        assert np.array_equal(gmin[k], z[f"gmin__{key}"], equal_nan=True), key
        assert (u[k, n:] == 0).all() and (v[k, n:] == 0).all(), key  # written, not the NaN of the input


def test_every_instance_of_the_batch_equals_its_batch_of_one():
    names, mats, us, vs = fixture_batch()
    u, v, gmin, rounds, _ = raw_project(pack(mats, "packed"), us, vs, 3, -1e-3)
    for k, C in enumerate(mats):
        n = C.shape[0]
        u1, v1, g1, r1, ret1 = raw_project(pack([C], "packed"), [us[k]], [vs[k]], 3, -1e-3)
        assert same(u1[0], u[k, :n]) and same(v1[0], v[k, :n]) and same(g1[0], gmin[k]), names[k]
        assert r1[0] == rounds[k] and ret1[0] == 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shift", (True, False))
def test_fixture_cases_reduce_costs_and_feasibility(layout, shift):
    z = cases()
    names, mats, us, vs = fixture_batch()
    p = pack(mats, layout)
    out, gmin, ret = raw_reduce(p, us, vs, shift)
    assert (ret == 0).all()
    stored = {str(k) for k in z["reduced_cases"]}
    for k, c in enumerate(names):
        key = case_key(*c)
        want, m = np_reduce(mats[k], us[k], vs[k], shift)
        assert np.array_equal(gmin[k], m, equal_nan=True), key
        got = matrix_of(out, p, k)
        assert np.array_equal(got, want, equal_nan=True), key
        name = f"red_{'shift' if shift else 'noshift'}__{key}"
        if key in stored and name in z.files:
            assert np.array_equal(got, z[name], equal_nan=True), key
        assert bool(z[f"feasible__{key}"]) == (not gmin[k] < -1e-8), key
    if layout == "padded":  # the padding of `out` is not touched
        block = out.reshape(len(mats), p.N, p.N)
        for k, C in enumerate(mats):
            n = C.shape[0]
            assert np.isnan(block[k, n:]).all() and np.isnan(block[k, :n, n:]).all()
    _, gmin2, ret2 = raw_reduce(p, us, vs, shift, want_matrix=False)  # the feasibility check: no matrix
    assert same(gmin2, gmin) and (ret2 == 0).all()


# --------------------------------------------------------------------------- against the uniform entries
def row_width():
    src = (PKG / "csrc" / "ragged_batch.hip").read_text()
    return int(re.search(r"constexpr int kRowThreads = (\d+);", src).group(1))


@functools.lru_cache(maxsize=None)
def shape_batch(family):
    """Sizes where the sweeps change shape: one and two elements, one element per thread of a row workgroup less
    one, exactly, plus one, two per thread plus one (the paired loads: one sweep plus one), and 513 mixed with
    64.  Seeds: infeasible, so that every round moves something."""
    w = row_width()
    sizes = (1, 2, w - 1, w, w + 1, 2 * w + 1, 513, 64)
    rs = np.random.RandomState([7, ("uniform", "integer").index(family)])
    mats, us, vs = [], [], []
    for n in sizes:
        C = rs.uniform(0, 1, (n, n)) if family == "uniform" else rs.randint(0, 5, (n, n)).astype(np.float64)
        C.setflags(write=False)
        mats.append(C)
        us.append(rs.uniform(0, 1, n))
        vs.append(rs.uniform(0, 1, n))
    return tuple(mats), tuple(us), tuple(vs)


@functools.lru_cache(maxsize=None)
def uniform_duals_reference(family):
    """The uniform entries on every instance alone: computed once, shared, never modified."""
    import torch

    from lap import _hip
    from solvers import project_feasible
    lib = _hip.require_device()
    mats, us, vs = shape_batch(family)
    out = []
    for C, u0, v0 in zip(mats, us, vs):
        n = C.shape[0]
        Cd, ud, vd = (torch.from_numpy(x.copy()).cuda() for x in (C, u0, v0))
        rm = torch.empty(n, dtype=torch.float64, device="cuda")
        assert lib.lapwarm_rowmin_batched(Cd.data_ptr(), 1, n, vd.data_ptr(), rm.data_ptr(), None) == 0
        rm0 = torch.empty(n, dtype=torch.float64, device="cuda")
        assert lib.lapwarm_rowmin_batched(Cd.data_ptr(), 1, n, None, rm0.data_ptr(), None) == 0
        red = torch.empty_like(Cd)
        g = torch.empty(1, dtype=torch.float64, device="cuda")
        nb = int(lib.lapwarm_sweep_workspace_bytes(1, n))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        assert lib.lapwarm_reduce_costs_batched(Cd.data_ptr(), 1, n, ud.data_ptr(), vd.data_ptr(), 1, red.data_ptr(),
                                                g.data_ptr(), ws.data_ptr(), nb, None) == 0
        torch.cuda.synchronize()
        pu, pv = project_feasible(C, u0, v0, max_rounds=3, tol=-1e-3)
        out.append(dict(rowmin=rm.cpu().numpy(), rowmin0=rm0.cpu().numpy(), red=red.cpu().numpy(),
                        gmin=float(g.cpu()), pu=pu, pv=pv))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", ("uniform", "integer"))
def test_prefix_is_bit_equal_to_the_uniform_entries_where_the_sweeps_change_shape(family, layout):
    mats, us, vs = shape_batch(family)
    p = pack(mats, layout)
    if layout == "packed":  # odd sizes: some bases are 8-byte aligned and no more
        bases = [p.C.data_ptr() + 8 * o for o in p.offsets.tolist()]
        assert any(a % 16 for a in bases) and all(a % 8 == 0 for a in bases)
    want = uniform_duals_reference(family)
    rm, ret = raw_rowmin(p, vs)
    rm0, _ = raw_rowmin(p)
    u, v, gmin, rounds, _ = raw_project(p, us, vs, 3, -1e-3)
    red, g, _ = raw_reduce(p, us, vs, True)
    assert (ret == 0).all() and rounds.max() == 3
    for k, (C, w) in enumerate(zip(mats, want)):
        n = C.shape[0]
        assert rounds[k] == np_project(C, us[k], vs[k], 3, -1e-3)[3], n
        assert np.array_equal(rm[k, :n], w["rowmin"]) and (rm[k, n:] == 0).all(), n
        assert np.array_equal(rm0[k, :n], w["rowmin0"]) and np.array_equal(rm0[k, :n], C.min(axis=1)), n
        assert np.array_equal(u[k, :n], w["pu"]) and np.array_equal(v[k, :n], w["pv"]), n
        assert gmin[k] == np_reduce(C, w["pu"], w["pv"], False)[1], n
        assert np.array_equal(matrix_of(red, p, k), w["red"]) and g[k] == w["gmin"], n


# --------------------------------------------------------------------------- sizes the device rejects
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bad_sizes_are_reported_and_leave_the_neighbours_alone(layout):
    names, mats, us, vs = fixture_batch()
    pick = [k for k, c in enumerate(names) if c[0] in ("uni", "nan") and c[2] == "infeas"]
    mats, us, vs = [mats[k] for k in pick], [us[k] for k in pick], [vs[k] for k in pick]
    p = pack(mats, layout)
    good = list(p.host_sizes)
    bad = list(good)
    bad[1], bad[4] = 0, p.N + 1
    ref = raw_project(p, us, vs, 3, -1e-3), raw_reduce(p, us, vs, True), raw_rowmin(p, vs)
    got = raw_project(p, us, vs, 3, -1e-3, sizes=bad), raw_reduce(p, us, vs, True, sizes=bad), \
        raw_rowmin(p, vs, sizes=bad)
    (u, v, gmin, rounds, ret), (red, g, rret), (rm, mret) = got
    for k in range(len(mats)):
        if k in (1, 4):
            assert ret[k] == 2 and rret[k] == 2 and mret[k] == 2
            assert (u[k] == 0).all() and (v[k] == 0).all() and gmin[k] == 0 and rounds[k] == 0
            assert g[k] == 0 and (rm[k] == 0).all()
            assert np.isnan(matrix_of(red, p, k)).all()  # an extent nobody knows: not written
        else:
            assert ret[k] == 0 and rret[k] == 0 and mret[k] == 0
            for a, b in zip(got[0] + got[1][1:] + got[2], ref[0] + ref[1][1:] + ref[2]):
                assert same(a[k], b[k]), k
            assert same(matrix_of(red, p, k), matrix_of(ref[1][0], p, k)), k


# ------------------------------------------------------------------------------------------- Python surface
def test_pipeline_entries_are_the_raw_calls(pipe):
    import torch

    from gnn import row_min_ragged
    names, mats, us, vs = fixture_batch()
    p = pack(mats, "packed")
    ud, vd = pad_vectors(us, p.N, 0.0), pad_vectors(vs, p.N, 0.0)
    u0, v0 = ud.clone(), vd.clone()
    u, v, gmin, rounds, ret = pipe.project_feasible_ragged(p, ud, vd, max_rounds=3, tol=-1e-3)
    # the inputs are left as they are (compared as bits: some seeds hold NaN)
    assert torch.equal(ud.view(torch.int64), u0.view(torch.int64))
    assert torch.equal(vd.view(torch.int64), v0.view(torch.int64))
    want = raw_project(p, us, vs, 3, -1e-3)
    for a, b in zip((u, v, gmin, rounds, ret), want):
        assert same(a.cpu().numpy(), b)
    out, g, _ = pipe.reduce_costs_ragged(p, ud, vd, shift_nonneg=True)
    wout, wg, _ = raw_reduce(p, us, vs, True)
    assert same(out.cpu().numpy(), wout) and same(g.cpu().numpy(), wg)
    assert pipe.reduce_costs_ragged(p, ud, vd, want_matrix=False)[0] is None
    feas = pipe.dual_feasible_ragged(p, ud, vd)
    z = cases()
    assert feas.dtype == torch.bool and feas.tolist() == [bool(z[f"feasible__{case_key(*c)}"]) for c in names]
    assert same(row_min_ragged(p, vd).cpu().numpy(), raw_rowmin(p, vs)[0])


def test_many_functions_against_the_fixture(pipe):
    import solvers
    z = cases()
    names, mats, us, vs = fixture_batch()
    got = solvers.project_feasible_many(mats, us, vs, max_rounds=3, tol=-0.5)
    for c, (u, v) in zip(names, got):
        key = case_key(*c)
        r = int(z[f"rounds__{key}"][2, 2])
        assert np.array_equal(u, z[f"u__{key}__r{r}"], equal_nan=True), key
        assert np.array_equal(v, z[f"v__{key}__r{r}"], equal_nan=True), key
    finite = [k for k, c in enumerate(names) if c[0] in ("uni", "int")]
    pu = [got[k][0] for k in finite]
    pv = [got[k][1] for k in finite]
    fm = [mats[k] for k in finite]
    assert solvers.check_dual_feasible_many(fm, pu, pv) is True
    first_bad = next(k for k, c in enumerate(names) if not bool(z[f"feasible__{case_key(*c)}"]))
    with pytest.raises(AssertionError, match=rf"Dual infeasible: min reduced cost .* < -tol \(instance {first_bad}\)"):
        solvers.check_dual_feasible_many(mats[:first_bad + 3], us[:first_bad + 3], vs[:first_bad + 3])
    stored = [str(k) for k in z["reduced_cases"]]
    index = {case_key(*c): k for k, c in enumerate(names)}
    ks = [index[key] for key in stored]
    reds = solvers.reduce_costs_many([mats[k] for k in ks], [us[k] for k in ks], [vs[k] for k in ks])
    for key, red in zip(stored, reds):
        assert np.array_equal(red, z[f"red_shift__{key}"], equal_nan=True), key


def test_classical_and_noisy_seeds_of_many_instances_have_the_reference_bits(pipe):
    import solvers
    z = cases()
    kinds_sizes = [(str(k), int(n)) for n in z["sizes"] for k in z["kinds"]]
    got = solvers.seed_row_col_minima_many([matrix(k, n) for k, n in kinds_sizes])
    for (k, n), (u, v) in zip(kinds_sizes, got):
        assert np.array_equal(u, z[f"rcseed_u__{k}_n{n}"], equal_nan=True), (k, n)
        assert np.array_equal(v, z[f"rcseed_v__{k}_n{n}"], equal_nan=True), (k, n)
    sizes = [int(n) for n in z["noisy_sizes"]]
    got = solvers.seed_noisy_optimal_many([matrix("opt", n) for n in sizes], noise_std=0.05,
                                          rng=np.random.default_rng(int(z["noisy_seed"])), pipeline=pipe)
    for n, (u, v) in zip(sizes, got):
        assert np.array_equal(u, z[f"noisyopt_u__n{n}"]) and np.array_equal(v, z[f"noisyopt_v__n{n}"]), n


def test_noisy_duals_ragged(pipe):
    import torch
    sizes = (7, 33, 64, 65, 33, 2)
    mats = [matrix("uni", n) for n in sizes]
    p = pack(mats, "packed")
    u, v = pipe.seed_row_col_minima_ragged(p)[:2]

    def run(seed, prob):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return pipe.noisy_duals_ragged(p, u, v, 0.15, generator=g, prob=prob)

    un, vn, hit = run(11, 1.0)
    assert hit.all() and pipe.dual_feasible_ragged(p, un, vn, tol=1e-12).all()
    for b, n in enumerate(sizes):
        assert not torch.equal(un[b, :n], u[b, :n]) and (un[b, n:] == 0).all() and (vn[b, n:] == 0).all()
    un2, vn2, _ = run(11, 1.0)
    assert torch.equal(un, un2) and torch.equal(vn, vn2)
    un3, _, _ = run(12, 1.0)
    assert not torch.equal(un, un3)
    u0, v0, hit0 = run(11, 0.0)
    assert not hit0.any() and torch.equal(u0, u) and torch.equal(v0, v)
    um, vm, hitm = run(5, 0.5)  # some instances: the others keep their bits, the perturbed ones are feasible
    for b in range(len(sizes)):
        if not bool(hitm[b]):
            assert torch.equal(um[b], u[b]) and torch.equal(vm[b], v[b])
    assert pipe.dual_feasible_ragged(p, um, vm, tol=1e-12).all()


def test_training_batch_with_noisy_labels(pipe):
    import torch

    from gnn.losses import warmstart_loss
    mats = [matrix("opt", n) for n in (7, 33, 64, 65)]
    clean = pipe.training_batch(mats)
    same_path = pipe.training_batch(mats, dual_noise_std=0.15, dual_noise_prob=0.0)
    for name in ("mask", "row_feat", "topk", "cost", "sizes", "u", "v"):
        assert torch.equal(getattr(clean, name), getattr(same_path, name)), name
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    noisy = pipe.training_batch(mats, dual_noise_std=0.15, dual_noise_prob=1.0, generator=g)
    for name in ("mask", "row_feat", "topk", "cost", "sizes"):
        assert torch.equal(getattr(clean, name), getattr(noisy, name)), name
    assert noisy.u.dtype == torch.float32 and noisy.u.shape == clean.u.shape
    # the fp64 labels behind the batch: the same draws from the same generator seed
    duals = pipe.oracle_duals_many(mats)
    g.manual_seed(3)
    p = pack(mats, "packed")
    u64, v64, hit = pipe.noisy_duals_ragged(p, duals.u, duals.v, 0.15, generator=g, prob=1.0)
    assert hit.all() and torch.equal(u64.float(), noisy.u) and torch.equal(v64.float(), noisy.v)
    assert pipe.dual_feasible_ragged(p, u64, v64, tol=1e-8).all()  # feasible for the float64 costs
    for b, C in enumerate(mats):
        n = C.shape[0]
        assert not torch.equal(noisy.u[b, :n], clean.u[b, :n])
        assert (noisy.u[b, n:] == 0).all() and (noisy.v[b, n:] == 0).all()
        # the float32 labels: each is within half an ulp, 2^-24 relative, of its fp64 value
        u, v = noisy.u[b, :n].double().cpu().numpy(), noisy.v[b, :n].double().cpu().numpy()
        slack = 2.0 ** -24 * (np.abs(u).max() + np.abs(v).max())
        assert ((C - u[:, None]) - v[None, :]).min() >= -1e-8 - slack, b
    u_pred = torch.zeros_like(noisy.u, requires_grad=True)
    loss, _ = warmstart_loss(noisy.cost, u_pred, noisy.u, noisy.mask)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(u_pred.grad).all()
