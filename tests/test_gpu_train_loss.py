"""The OneGNN training loss on the MI355X (csrc/train_loss.hip through the C ABI and gnn.losses) against the
reference's outcomes in tests/golden/train_loss_cases.npz and the NumPy restatement of train_loss_common.py.

dual_lower, feas, u_reg and grad_u are rounded once from an fp64 accumulation of the float32 terms, so they lie
within 1 float32 ulp of the stored float64 values (the fp64 accumulation error and the float32 grad_scale 1/B
stay below half an ulp together); everything else is exact."""
import ctypes as ct

import numpy as np
import pytest

import train_loss_common as tl

pytestmark = pytest.mark.gpu

CASES = tl.TrainLossCases()
ALL = list(range(len(CASES)))
LABELS = CASES.labels()
MIXED = LABELS.index("uniform-n65-mixed")


SENTINEL = 0x5AA55AA5  # what run_abi(tail=True) pre-fills every output with, as int32 bits


def run_abi(m, sizes=None, stream=None, ws=None, tail=False, cost_offset=0):
    """lapwarm_train_loss_forward and _backward on case m; everything back as NumPy arrays.

    tail: v, arow, assign and grad get n more elements and terms and ret one more row, everything pre-filled
    with SENTINEL; the extra elements must come back untouched.  cost_offset: cost starts that many bytes (a
    multiple of 4) into its allocation."""
    import torch

    from lap import _hip
    lib = _hip.require_device()
    dev = torch.device("cuda:0")
    B, n = m["u_pred"].shape
    assert cost_offset % 4 == 0
    buf = torch.empty((B * n * n + cost_offset // 4,), dtype=torch.float32, device=dev)
    cost = buf[cost_offset // 4:].view(B, n, n)
    cost.copy_(torch.from_numpy(m["cost"]))
    assert buf.data_ptr() % 16 == 0 and cost.data_ptr() == buf.data_ptr() + cost_offset
    u = torch.from_numpy(m["u_pred"]).to(dev)
    t = torch.from_numpy(m["u_target"]).to(dev)
    sz = torch.from_numpy(np.asarray(m["sizes"] if sizes is None else sizes, dtype=np.int32)).to(dev)
    w = torch.tensor(tl.WEIGHTS, dtype=torch.float32, device=dev)

    def output(count, extra, dtype):
        if not tail:
            return torch.empty((count,), dtype=dtype, device=dev)
        return torch.full((count + extra,), SENTINEL, dtype=torch.int32, device=dev).view(dtype)

    flat = dict(v=output(B * n, n, torch.float32), arow=output(B * n, n, torch.int32),
                assign=output(B * n, n, torch.int32), terms=output(B * 4, 4, torch.float32),
                ret=output(B, 1, torch.int32), grad=output(B * n, n, torch.float32))
    counts = dict(v=B * n, arow=B * n, assign=B * n, terms=B * 4, ret=B, grad=B * n)
    shapes = dict(v=(B, n), arow=(B, n), assign=(B, n), terms=(B, 4), ret=(B,), grad=(B, n))
    v, arow, assign, terms, ret, grad = (flat[k][:counts[k]].view(shapes[k])
                                         for k in ("v", "arow", "assign", "terms", "ret", "grad"))
    nbytes = int(lib.lapwarm_train_loss_workspace_bytes(B, n))
    assert nbytes > 0
    if ws is None:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    assert ws.numel() >= nbytes
    s = torch.cuda.current_stream(dev) if stream is None else stream
    s.wait_stream(torch.cuda.current_stream(dev))
    rc = lib.lapwarm_train_loss_forward(cost.data_ptr(), B, n, sz.data_ptr(), u.data_ptr(), t.data_ptr(),
                                        v.data_ptr(), arow.data_ptr(), assign.data_ptr(), terms.data_ptr(),
                                        ret.data_ptr(), ws.data_ptr(), ws.numel(), ct.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, _hip.last_error())
    rc = lib.lapwarm_train_loss_backward(B, n, sz.data_ptr(), u.data_ptr(), t.data_ptr(), w.data_ptr(), 1.0 / B,
                                         grad.data_ptr(), ws.data_ptr(), ws.numel(), ct.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, _hip.last_error())
    s.synchronize()
    if tail:
        for key, x in flat.items():
            beyond = x[counts[key]:].view(torch.int32).cpu().numpy()
            assert (beyond == SENTINEL).all(), (key, "written beyond its end at", np.flatnonzero(beyond != SENTINEL)[:8])
    out = dict(v=v, arow=arow, assign=assign, terms=terms, ret=ret, grad=grad)
    out = {k: x.cpu().numpy() for k, x in out.items()}
    out["ws"] = ws
    return out


@pytest.fixture(scope="module")
def device_results():
    """Forward and backward of every golden case, run once and shared; nothing modifies them."""
    return [run_abi(CASES.case(k)) for k in ALL]


@pytest.mark.parametrize("k", ALL, ids=LABELS)
def test_exact_outputs(k, device_results):
    m, r, d = CASES.case(k), CASES.restated(k), device_results[k]
    assert (d["ret"] == 0).all()
    assert tl.bits_equal32(d["v"], m["ref_v"])
    assert np.array_equal(d["arow"], r["a"])
    assert np.array_equal(d["assign"], r["assign"]) and np.array_equal(d["assign"], m["assign"])
    assert tl.bits_equal32(d["terms"][:, 3], r["primal_upper"])
    if m["primal_equal"]:
        assert tl.bits_equal32(d["terms"][:, 3], m["ref_primal"])
    for b, nb in enumerate(m["sizes"]):
        assert (d["assign"][b, nb:] == -1).all() and (d["arow"][b, nb:] == -1).all()
        assert (d["v"][b, nb:] == 0).all()


@pytest.mark.parametrize("k", ALL, ids=LABELS)
def test_sums_and_gradient_within_one_ulp(k, device_results):
    m, d = CASES.case(k), device_results[k]
    for col, key in enumerate(("dual64", "feas64", "ureg64")):
        print(key, d["terms"][:, col], m[key])
        assert tl.within_one_ulp(d["terms"][:, col], m[key]).all(), key
    err = np.abs(d["grad"].astype(np.float64) - m["g64"]) / tl.ulp32(m["g64"])
    print("grad_u: largest error in ulp", err[m["g64"] != 0].max(initial=0.0))
    assert tl.within_one_ulp(d["grad"], m["g64"]).all()
    for b, nb in enumerate(m["sizes"]):
        assert (d["grad"][b, nb:] == 0).all()


def test_partly_filled_batch_on_the_wide_load_path():
    """n = 64 takes the 16-byte loads; sizes that are no multiple of 4 end inside a lane's four columns."""
    m = dict(CASES.case(LABELS.index("uniform-n64-B3")))
    m["sizes"] = np.array([64, 33, 7], dtype=np.int32)
    r = tl.restate(m["cost"], m["u_pred"], m["u_target"], m["sizes"])
    d = run_abi(m)
    assert (d["ret"] == 0).all()
    assert tl.bits_equal32(d["v"], r["v"]) and np.array_equal(d["arow"], r["a"])
    assert np.array_equal(d["assign"], r["assign"]) and tl.bits_equal32(d["terms"][:, 3], r["primal_upper"])
    for col, key in enumerate(("dual64", "feas64", "ureg64")):
        assert tl.within_one_ulp(d["terms"][:, col], r[key]).all(), key
    assert tl.within_one_ulp(d["grad"], r["g64"]).all()


def test_bad_size_is_reported_and_leaves_the_neighbours_alone(device_results):
    m, d = CASES.case(MIXED), device_results[MIXED]
    sizes = m["sizes"].copy()
    for bad in (0, m["u_pred"].shape[1] + 1, -3):
        sizes[2] = bad
        e = run_abi(m, sizes=sizes)
        assert e["ret"].tolist() == [0, 0, 2, 0]
        assert np.isnan(e["terms"][2]).all()
        assert (e["assign"][2] == -1).all() and (e["grad"][2] == 0).all()
        keep = [0, 1, 3]
        for key in ("v", "arow", "assign", "terms", "grad"):
            assert np.array_equal(e[key][keep].view(np.int32), d[key][keep].view(np.int32)), key


def test_other_stream_and_reused_workspace(device_results):
    import torch
    k = LABELS.index("uniform-n257-B3")
    m, d = CASES.case(k), device_results[k]
    from lap import _hip
    # a workspace full of leftovers: a word that is read without being written inside the call shows
    nbytes = int(_hip.require_device().lapwarm_train_loss_workspace_bytes(*m["u_pred"].shape))
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    e = run_abi(m, stream=torch.cuda.Stream(torch.device("cuda:0")), ws=ws)
    f = run_abi(m, ws=e["ws"])
    for key in ("v", "arow", "assign", "terms", "grad", "ret"):
        assert np.array_equal(e[key].view(np.int32), d[key].view(np.int32)), key
        assert np.array_equal(f[key].view(np.int32), d[key].view(np.int32)), key


def test_abi_argument_codes():
    from lap import _hip
    lib = _hip.require_device()
    assert lib.lapwarm_train_loss_workspace_bytes(1, 16385) == 0
    assert lib.lapwarm_train_loss_forward(None, 1, 16385, None, None, None, None, None, None, None, None, None, 0,
                                          None) == -5
    assert lib.lapwarm_train_loss_forward(None, 0, 8, None, None, None, None, None, None, None, None, None, 0,
                                          None) == -2
    assert lib.lapwarm_train_loss_forward(None, 2, 8, None, None, None, None, None, None, None, None, None, 16,
                                          None) == -1
    assert lib.lapwarm_train_loss_backward(2, 8, None, None, None, None, 1.0, None, None, 16, None) == -1
    assert lib.lapwarm_train_loss_backward(2, 16385, None, None, None, None, 1.0, None, None, 16, None) == -5


def test_warmstart_loss_backward_is_the_kernel_gradient(device_results):
    """Through OneGNN in training mode: loss.backward() gives bit for bit the parameter gradients of
    u.backward(g) with g from lapwarm_train_loss_backward; the Function adds nothing of its own."""
    import torch

    from gnn import OneGNN
    from gnn.losses import greedy_primal_upper_batch, warmstart_loss
    m, d = CASES.case(MIXED), device_results[MIXED]
    dev = torch.device("cuda:0")
    B, n = m["u_pred"].shape
    torch.manual_seed(0)
    model = OneGNN(21, hidden=64, layers=2, dropout=0.0).to(dev).train()
    feat = torch.randn(B, n, 21, device=dev)
    cost = torch.from_numpy(m["cost"]).to(dev)
    target = torch.from_numpy(m["u_target"]).to(dev)
    mask = torch.arange(n, device=dev)[None, :] < torch.from_numpy(m["sizes"].astype(np.int64)).to(dev)[:, None]

    u1 = model(feat, cost=cost, mask=mask)["u"]
    loss, metrics = warmstart_loss(cost, u1, target, mask)
    loss.backward()
    got = [p.grad.detach().clone() for p in model.parameters()]
    assert all(g is not None for g in got) and any(bool((g != 0).any()) for g in got)
    assert set(metrics) >= {"primal_gap", "feas", "dual_lower", "primal_upper", "u_reg", "v_proj", "assign"}
    assert all(t.is_cuda for t in metrics.values()) and not metrics["primal_gap"].requires_grad

    model.zero_grad(set_to_none=True)
    u2 = model(feat, cost=cost, mask=mask)["u"]
    assert torch.equal(u1.detach(), u2.detach())
    case = dict(cost=m["cost"], u_pred=u2.detach().cpu().numpy(), u_target=m["u_target"], sizes=m["sizes"])
    e = run_abi(case)
    u2.backward(torch.from_numpy(e["grad"]).to(dev))
    want = [p.grad for p in model.parameters()]
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))

    # the loss is the reference's combination of the per-instance terms, and the metrics are the kernel's
    terms = torch.from_numpy(e["terms"]).to(dev)
    gap = terms[:, 3] - terms[:, 0]
    ref_loss = gap.mean() + terms[:, 1].mean() + 0.1 * terms[:, 2].mean()
    assert torch.equal(loss.detach(), ref_loss)
    assert torch.equal(metrics["primal_gap"], gap) and torch.equal(metrics["primal_upper"], terms[:, 3])
    assert np.array_equal(metrics["assign"].cpu().numpy(), e["assign"])
    assert np.array_equal(metrics["v_proj"].cpu().numpy().view(np.int32), e["v"].view(np.int32))

    # the evaluation metric is the loss's primal_upper; half-precision u is upcast
    pu, assign = greedy_primal_upper_batch(cost, u2.detach(), mask)
    assert torch.equal(pu, terms[:, 3]) and np.array_equal(assign.cpu().numpy(), e["assign"])
    full = torch.from_numpy(CASES.case(LABELS.index("uniform-n64-B3"))["cost"]).to(dev)
    uf = torch.from_numpy(CASES.case(LABELS.index("uniform-n64-B3"))["u_pred"]).to(dev)
    pu, assign = greedy_primal_upper_batch(full, uf)
    k64 = LABELS.index("uniform-n64-B3")
    assert np.array_equal(pu.cpu().numpy().view(np.int32), device_results[k64]["terms"][:, 3].view(np.int32))
    assert np.array_equal(assign.cpu().numpy(), device_results[k64]["assign"])
    half = u2.detach().to(torch.bfloat16).requires_grad_()
    loss_h, _ = warmstart_loss(cost, half, target, mask)
    loss_h.backward()
    assert half.grad.dtype == torch.bfloat16 and bool(torch.isfinite(loss_h))
