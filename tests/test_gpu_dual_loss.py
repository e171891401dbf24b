"""The DualGNN training loss on the MI355X (csrc/train_loss.hip through the C ABI and gnn.losses.dual_warmstart_loss)
against the NumPy restatement of dual_loss_common.py: on the stored cases of tests/golden/dual_loss_cases.npz, on the
cases of train_loss_common.LARGE_SPECS that reach each kernel shape (regenerated, v_hint in the place of u_target),
and on built cases for the per-row sum S_i: one row that owns every column, every row owning its own, an instance of
size 0 between two others.

v_proj, argmin_row, assign, ret and primal_upper are exact.  dual_lower, feas, v_reg, grad_u and grad_v_hint are
rounded once from an fp64 evaluation, so they lie within 1 float32 ulp of the fp64 restatement; grad_u is allowed
the fp64 summation bound of its run of S_i on top (dual_loss_common.grad_u_allowance), because S_i can cancel.

The issue writes the one-segment case as "u_0 = -50".  With v_j = min_i (C_ij - u_i) it is u_0 = +50 that makes row
0 attain every column minimum; the case is built with +50 and asserts what it is there for, cnt_0 = n_b."""
import ctypes as ct

import numpy as np
import pytest

import dual_loss_common as dl
import test_gpu_train_loss as one_loss
import train_loss_common as tl

pytestmark = pytest.mark.gpu

CASES = dl.DualLossCases()
ALL = list(range(len(CASES)))
LABELS = CASES.labels()
LARGE = ("uniform-n1028-mixed", "integer-n1025-B2", "inf-n1028-B2", "uniform-n4100-mixed")
BUILT_N = (257, 1025)
SENTINEL = 0x5AA55AA5


def run_abi(m, stream=None, ws=None, u_pred=None):
    """lapwarm_dual_loss_forward and _backward on case m; everything back as NumPy arrays.  Every output has n more
    elements (terms and ret one more row) pre-filled with SENTINEL, which must come back untouched."""
    import torch

    from lap import _hip
    lib = _hip.require_device()
    dev = torch.device("cuda:0")
    B, n = m["u_pred"].shape
    cost = torch.from_numpy(np.ascontiguousarray(m["cost"])).to(dev)
    u = torch.from_numpy(m["u_pred"] if u_pred is None else u_pred).to(dev)
    vh = torch.from_numpy(m["v_hint"]).to(dev)
    sz = torch.from_numpy(np.asarray(m["sizes"], dtype=np.int32)).to(dev)
    w = torch.tensor(dl.WEIGHTS, dtype=torch.float32, device=dev)
    counts = dict(v=B * n, arow=B * n, assign=B * n, terms=B * 4, ret=B, grad=B * n, gvh=B * n)
    extra = dict(v=n, arow=n, assign=n, terms=4, ret=1, grad=n, gvh=n)
    dtypes = dict(v=torch.float32, arow=torch.int32, assign=torch.int32, terms=torch.float32, ret=torch.int32,
                  grad=torch.float32, gvh=torch.float32)
    shapes = dict(v=(B, n), arow=(B, n), assign=(B, n), terms=(B, 4), ret=(B,), grad=(B, n), gvh=(B, n))
    flat = {k: torch.full((counts[k] + extra[k],), SENTINEL, dtype=torch.int32, device=dev).view(dtypes[k])
            for k in counts}
    o = {k: flat[k][:counts[k]].view(shapes[k]) for k in counts}
    nbytes = int(lib.lapwarm_dual_loss_workspace_bytes(B, n))
    assert nbytes >= int(lib.lapwarm_train_loss_workspace_bytes(B, n)) > 0
    if ws is None:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    assert ws.numel() >= nbytes
    s = torch.cuda.current_stream(dev) if stream is None else stream
    s.wait_stream(torch.cuda.current_stream(dev))
    rc = lib.lapwarm_dual_loss_forward(cost.data_ptr(), B, n, sz.data_ptr(), u.data_ptr(), vh.data_ptr(),
                                       o["v"].data_ptr(), o["arow"].data_ptr(), o["assign"].data_ptr(),
                                       o["terms"].data_ptr(), o["ret"].data_ptr(), ws.data_ptr(), ws.numel(),
                                       ct.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, _hip.last_error())
    rc = lib.lapwarm_dual_loss_backward(B, n, sz.data_ptr(), u.data_ptr(), vh.data_ptr(), w.data_ptr(), 1.0 / B,
                                        o["grad"].data_ptr(), o["gvh"].data_ptr(), ws.data_ptr(), ws.numel(),
                                        ct.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, _hip.last_error())
    s.synchronize()
    for key, x in flat.items():
        beyond = x[counts[key]:].view(torch.int32).cpu().numpy()
        assert (beyond == SENTINEL).all(), (key, "written beyond its end at", np.flatnonzero(beyond != SENTINEL)[:8])
    out = {k: x.cpu().numpy() for k, x in o.items()}
    out["ws"] = ws
    return out


def check(m, r, d):
    """Every output of one run against the restatement r of its inputs."""
    sizes = np.asarray(m["sizes"])
    valid = sizes > 0
    assert np.array_equal(d["ret"], np.where(valid, 0, 2))
    assert tl.bits_equal32(d["v"], r["v"])
    assert np.array_equal(d["arow"], r["a"]) and np.array_equal(d["assign"], r["assign"])
    assert tl.bits_equal32(d["terms"][valid, 3], r["primal_upper"][valid])
    assert np.isnan(d["terms"][~valid]).all()
    for col, key in enumerate(("dual64", "feas64", "vreg64")):
        print(key, d["terms"][:, col], r[key])
        assert tl.within_one_ulp(d["terms"][valid, col], r[key][valid]).all(), key
    extra = dl.grad_u_allowance(r, sizes)
    err = np.abs(d["grad"].astype(np.float64) - r["g64"])
    print("grad_u: max error in ulps", (err / tl.ulp32(r["g64"])).max(), "largest allowance beyond one ulp", extra.max())
    assert dl.within_one_ulp_plus(d["grad"], r["g64"], extra).all()
    print("grad_v_hint: max error in ulps", (np.abs(d["gvh"] - r["gvh64"]) / tl.ulp32(r["gvh64"])).max())
    assert tl.within_one_ulp(d["gvh"], r["gvh64"]).all()
    for b, nb in enumerate(sizes):
        assert (d["grad"][b, nb:] == 0).all() and (d["gvh"][b, nb:] == 0).all()
        assert (d["v"][b, nb:] == 0).all() and (d["arow"][b, nb:] == -1).all() and (d["assign"][b, nb:] == -1).all()


@pytest.fixture(scope="module")
def device_results():
    """Forward and backward of every stored case, run once and shared; nothing modifies them."""
    return [run_abi(CASES.case(k)) for k in ALL]


@pytest.mark.parametrize("k", ALL, ids=LABELS)
def test_stored_cases(k, device_results):
    m, r, d = CASES.case(k), CASES.restated(k), device_results[k]
    check(m, r, d)
    assert tl.bits_equal32(d["v"], m["ref_v"])
    if m["primal_equal"]:
        assert tl.bits_equal32(d["terms"][:, 3], m["ref_primal"])


def as_dual(m):
    m = dict(m)
    m["v_hint"] = m.pop("u_target")
    return m


@pytest.mark.parametrize("label", LARGE)
def test_large_cases(label):
    m = as_dual(tl.large_case(label))
    r = dl.restate(m["cost"], m["u_pred"], m["v_hint"], m["sizes"])
    if label.startswith("integer"):
        assert (r["cnt"].max(axis=1) > 1).all()
    check(m, r, run_abi(m))


def built(kind, n):
    rng = np.random.default_rng(20250918 + n)
    if kind == "one-row-owns-all":
        sizes = np.asarray([n, n - 1], dtype=np.int32)
        cost, u, vh = tl.uniform_case(rng, 2, n, sizes)
        u[:, 0] = 50.0
    elif kind == "own-column":
        sizes = np.asarray([n, n - 3], dtype=np.int32)
        cost = np.broadcast_to(np.float32(10) * (1 - np.eye(n, dtype=np.float32)), (2, n, n)).copy()
        u = np.zeros((2, n), dtype=np.float32)
        vh = rng.uniform(-4.0, 4.0, size=(2, n)).astype(np.float32)
        tl.pad(cost, u, vh, sizes)
    else:
        sizes = np.asarray([n, 0, n - 3], dtype=np.int32)
        cost, u, vh = tl.uniform_case(rng, 3, n, sizes)
    return dict(cost=cost, u_pred=u, v_hint=vh, sizes=sizes)


@pytest.mark.parametrize("n", BUILT_N)
@pytest.mark.parametrize("kind", ("one-row-owns-all", "own-column", "size-0"))
def test_built_cases(kind, n):
    m = built(kind, n)
    r = dl.restate(m["cost"], m["u_pred"], m["v_hint"], m["sizes"])
    if kind == "one-row-owns-all":  # one run of length n_b; every other row owns nothing
        for b, nb in enumerate(m["sizes"]):
            assert r["cnt"][b, 0] == nb and (r["cnt"][b, 1:] == 0).all() and (r["S"][b, 1:] == 0).all()
    elif kind == "own-column":
        for b, nb in enumerate(m["sizes"]):
            assert np.array_equal(r["a"][b, :nb], np.arange(nb)) and (r["cnt"][b, :nb] == 1).all()
    d = run_abi(m)
    check(m, r, d)
    if kind == "size-0":
        assert d["ret"].tolist() == [0, 2, 0] and (d["grad"][1] == 0).all() and (d["gvh"][1] == 0).all()
        # the neighbours are what they are alone
        for b in (0, 2):
            alone = {k: x[b:b + 1] for k, x in m.items()}
            da = run_abi(alone)
            for key in ("v", "arow", "assign", "terms"):
                assert np.array_equal(d[key][b].view(np.int32), da[key][0].view(np.int32)), key
            # (the gradients carry grad_scale 1 / B of their own batch: compared through the restatement above)


def test_determinism_and_a_reused_workspace_on_another_stream():
    import torch
    m = as_dual(tl.large_case("integer-n1025-B2"))
    first = run_abi(m)
    again = run_abi(m)
    side = torch.cuda.Stream()
    reused = run_abi(m, stream=side, ws=first["ws"])
    for key in ("v", "arow", "assign", "terms", "ret", "grad", "gvh"):
        for other in (again, reused):
            assert np.array_equal(first[key].view(np.int32), other[key].view(np.int32)), key


@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_autograd_returns_the_kernels_gradients(dtype):
    import torch

    from gnn.losses import dual_warmstart_loss
    k = LABELS.index("uniform-n64-mixed")
    m = CASES.case(k)
    dev = torch.device("cuda:0")
    td = getattr(torch, dtype)
    u = torch.from_numpy(m["u_pred"]).to(dev).to(td).requires_grad_()
    vh = torch.from_numpy(m["v_hint"]).to(dev).requires_grad_()
    n = u.shape[1]
    mask = torch.arange(n, device=dev)[None, :] < torch.from_numpy(m["sizes"]).to(dev)[:, None]
    loss, metrics = dual_warmstart_loss(torch.from_numpy(m["cost"]).to(dev), u, vh, mask)
    loss.backward()
    torch.cuda.synchronize()
    d = run_abi(m, u_pred=u.detach().to(torch.float32).cpu().numpy())
    assert u.grad.dtype == td and vh.grad.dtype == torch.float32
    want_u = torch.from_numpy(d["grad"]).to(td)
    assert torch.equal(u.grad.cpu(), want_u) and tl.bits_equal32(vh.grad.cpu().numpy(), d["gvh"])
    assert set(metrics) == {"primal_gap", "feas", "dual_lower", "primal_upper", "v_reg", "v_proj", "assign",
                            "argmin_row", "ret"}
    assert tl.bits_equal32(metrics["v_reg"].cpu().numpy(), d["terms"][:, 2])
    assert tl.bits_equal32(metrics["v_proj"].cpu().numpy(), d["v"])
    t = torch.from_numpy(d["terms"])
    want = (t[:, 3] - t[:, 0]).mean() + t[:, 1].mean() + torch.tensor(0.1) * t[:, 2].mean()
    assert abs(float(loss.detach()) - float(want)) <= 4 * tl.ulp32(float(want))


def test_the_onegnn_entries_are_not_disturbed():
    """The outputs of the OneGNN entries on a stored train_loss case, before and after a dual-loss call that
    shares nothing with them: the shared kernels and the workspace layout they see are the same."""
    k = one_loss.MIXED
    m = one_loss.CASES.case(k)
    before = one_loss.run_abi(m, tail=True)
    run_abi(CASES.case(LABELS.index("uniform-n64-mixed")))
    after = one_loss.run_abi(m, tail=True)
    for key in ("v", "arow", "assign", "terms", "ret", "grad"):
        assert np.array_equal(before[key].view(np.int32), after[key].view(np.int32)), key
    r = one_loss.CASES.restated(k)
    assert np.array_equal(after["arow"], r["a"]) and tl.within_one_ulp(after["grad"], m["g64"]).all()
