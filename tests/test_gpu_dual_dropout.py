"""DualGNN's fused dropout on the MI355X: the keep rule of the kernels against NumPy byte for byte, the four entries
with dropout against fp64 torch and autograd on the CPU with the same masks multiplied in, and DualGNN with
fused_dropout against the fp64 plain-path model whose two dropouts are replaced by those masks.

Tolerance, per output: refine_backward_common.tolerance, 4 x the max-abs error of PyTorch-CPU float32 of the same
formulation on the same masks against the fp64 reference, or 1e-6 * max(1, max|ref|) if that is larger.  The seeds are
those of dual_dropout_common, whose keep rates test_dual_dropout_host.py checks."""
import ctypes as ct

import numpy as np
import pytest
import torch

import dual_backward_common as dbc
import dual_dropout_common as ddc
import dual_gnn_common as dg
import test_gpu_dual_backward as tgb
from host_common import device_lib as lib  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = tgb.SENTINEL
P = ddc.P
_stream, _ptr, _compare = tgb._stream, tgb._ptr, tgb._compare


# ---- lapwarm_dual_dropout_keep ---------------------------------------------------------------------------------

@pytest.mark.parametrize("stream_id", [0, 1])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_the_keep_rule_of_the_kernels_is_the_numpy_one_byte_for_byte(lib, p, stream_id):
    first, count = ddc.KEEP_FIRST, ddc.KEEP_COUNT
    assert ddc.SEED_KEEP >> 63 == 1 and first > 2**34 and count % 4 and count % 64
    keep = torch.full((count + 64,), 7, dtype=torch.uint8, device=DEV)
    rc = lib.lapwarm_dual_dropout_keep(ddc.SEED_KEEP, stream_id, first, count, p, keep.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = keep.cpu().numpy()
    want = ddc.keep_range(ddc.SEED_KEEP, stream_id, first, count, p).astype(np.uint8)
    assert np.array_equal(got[:count], want)
    assert np.all(got[count:] == 7)  # nothing past the count is written


# ---- lapwarm_dual_edge_scores_dropout --------------------------------------------------------------------------

def _edge_forward(lib, d, sizes, B, N, heads, seed, p):
    """p None: the entries without dropout"""
    scores = torch.full((B, 2, heads, N, N), SENTINEL, device=DEV)
    ptrs = [t.data_ptr() for t in d]
    if p is None and sizes is None:
        rc = lib.lapwarm_dual_edge_scores(*ptrs, scores.data_ptr(), B, N, heads, _stream())
    elif p is None:
        rc = lib.lapwarm_dual_edge_scores_ragged(*ptrs, scores.data_ptr(), sizes.data_ptr(), B, N, heads, _stream())
    else:
        rc = lib.lapwarm_dual_edge_scores_dropout(*ptrs, scores.data_ptr(), _ptr(sizes), B, N, heads, seed, p, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return scores.cpu()


def test_edge_scores_with_dropout_against_fp64_on_tail_tiles(lib):
    (B, N), heads = ddc.EDGE_SHAPES[0], 4
    args, _ = dbc.edge_case(B, N, heads)
    mask0 = ddc.edge_mask(ddc.SEED_EDGE, P, B, N)
    want = ddc.edge_scores_torch(*[t.double() for t in args], mask0)
    yard = ddc.edge_scores_torch(*args, mask0)
    d = [t.to(DEV).contiguous() for t in args]
    got = _edge_forward(lib, d, None, B, N, heads, ddc.SEED_EDGE, P)
    _compare(f"edge scores B={B} N={N} p={P}", {"scores": got.numpy()}, {"scores": want}, {"scores": yard})
    plain = dg.edge_scores_torch(*[t.double() for t in args])
    assert dbc.max_err(got.numpy(), plain.numpy()) > 1e-3  # the masked reference is not the undropped output
    # equal inputs and an equal seed: equal bits; another seed: another mask
    assert torch.equal(got, _edge_forward(lib, d, None, B, N, heads, ddc.SEED_EDGE, P))
    assert not torch.equal(got, _edge_forward(lib, d, None, B, N, heads, ddc.SEED_EDGE + 1, P))
    # p = 0: the bits of the entry without dropout
    assert torch.equal(_edge_forward(lib, d, None, B, N, heads, ddc.SEED_EDGE, 0.0),
                       _edge_forward(lib, d, None, B, N, heads, 0, None))


def test_edge_scores_with_dropout_and_sizes_give_the_bits_of_the_uniform_call_on_the_prefixes(lib):
    sizes_host, heads = (5, 17, 12), 4
    B, N = ddc.EDGE_SHAPES[1]
    assert (B, N) == (len(sizes_host), max(sizes_host))
    args, _ = dbc.edge_case(B, N, heads)
    d = [t.to(DEV).contiguous() for t in args]
    sizes = torch.tensor(sizes_host, dtype=torch.int32, device=DEV)
    uniform = _edge_forward(lib, d, None, B, N, heads, ddc.SEED_EDGE, P)
    ragged = _edge_forward(lib, d, sizes, B, N, heads, ddc.SEED_EDGE, P)
    keep = dbc.prefix_mask(sizes_host, N)
    pair = (keep[:, :, None] & keep[:, None, :])[:, None, None].expand_as(uniform)
    assert torch.equal(ragged[pair], uniform[pair])
    assert bool((ragged[~pair] == SENTINEL).all())  # outside the prefixes nothing is written
    assert torch.equal(_edge_forward(lib, d, sizes, B, N, heads, ddc.SEED_EDGE, 0.0)[pair],
                       _edge_forward(lib, d, sizes, B, N, heads, 0, None)[pair])


# ---- lapwarm_dual_attention_stats_dropout and lapwarm_dual_attention_backward_dropout ------------------------

def _attention_forward(lib, d, mask8, sizes, B, N, H, D, seed, p):
    row_msg, col_msg = (torch.full((B, N, H * D), SENTINEL, device=DEV) for _ in range(2))
    rs, cs = (torch.full((B, H, N, 2), SENTINEL, device=DEV) for _ in range(2))
    rc = lib.lapwarm_dual_attention_stats_dropout(
        *[t.data_ptr() for t in d[:6]], _ptr(mask8), _ptr(sizes), d[6].data_ptr(), d[7].data_ptr(), row_msg.data_ptr(),
        col_msg.data_ptr(), rs.data_ptr(), cs.data_ptr(), B, N, H, D, seed, p, _stream())
    assert rc == 0
    return row_msg, col_msg, rs, cs


def _attention_backward(lib, d, g, mask8, sizes, B, N, H, D, seed, p, fill=0):
    fwd = _attention_forward(lib, d, mask8, sizes, B, N, H, D, seed, p)
    ws, nbytes = tgb._workspace(lib, B, N, H, fill)
    out = {"dS": torch.full((B, 2, H, N, N), SENTINEL, device=DEV)}
    for name in ("da_row", "dc_row", "da_col", "dc_col"):
        out[name] = torch.full((B, H, N), SENTINEL, device=DEV)
    out["dkb"] = torch.full((2 * H,), SENTINEL, device=DEV)
    out["d_row_val"], out["d_col_val"] = (torch.full((B, N, H * D), SENTINEL, device=DEV) for _ in range(2))
    rc = lib.lapwarm_dual_attention_backward_dropout(
        *[t.data_ptr() for t in d[:6]], _ptr(mask8), _ptr(sizes), d[6].data_ptr(), d[7].data_ptr(),
        *[t.data_ptr() for t in fwd], g[0].data_ptr(), g[1].data_ptr(),
        *[out[name].data_ptr() for name in dbc.ATT_NAMES], B, N, H, D, ws.data_ptr(), nbytes, seed, p, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in out.items()}, [t.cpu() for t in fwd]


def _dropped_attention_autograd(args, grads, mask1, dtype):
    scores, a_row, c_row, a_col, c_col, kbias, mask, row_val, col_val = args
    leaves = [t.detach().to(dtype).requires_grad_() for t in (scores, a_row, c_row, a_col, c_col, kbias, row_val, col_val)]
    s, ar, cr, ac, cc, kb, rv, cv = leaves
    rm, cm = ddc.attention_torch(s, ar, cr, ac, cc, kb, mask, rv, cv, mask1)
    ((rm * grads[0].to(dtype)).sum() + (cm * grads[1].to(dtype)).sum()).backward()
    return dict(zip(dbc.ATT_NAMES, (t.grad for t in leaves))), (rm.detach(), cm.detach())


@pytest.mark.parametrize("B,N,H,D", ddc.ATTN_SHAPES, ids=lambda v: str(v))
def test_attention_with_dropout_forward_statistics_and_all_eight_gradients(lib, B, N, H, D):
    """(65, 4, 8): two key tiles; (33, 2, 160): two passes over the keys for head_dim > 128, which must see one mask"""
    assert (N > 64 and D <= 128) or D > 128
    args, grads = dbc.attention_case(B, N, H, D, "prefix")
    mask = args[6]
    mask1 = ddc.attn_mask(ddc.SEED_ATTN, P, B, H, N)
    want, want_msgs = _dropped_attention_autograd(args, grads, mask1, torch.float64)
    yard, yard_msgs = _dropped_attention_autograd(args, grads, mask1, torch.float32)
    d = [t.to(DEV).contiguous() for t in args[:6] + args[7:]]
    g = [t.to(DEV).contiguous() for t in grads]
    mask8 = mask.to(torch.uint8).to(DEV).contiguous()
    label = f"attention B={B} N={N} H={H} D={D} p={P}"
    got, fwd = _attention_backward(lib, d, g, mask8, None, B, N, H, D, ddc.SEED_ATTN, P)
    _compare(label + " forward", {"row_msg": fwd[0].numpy(), "col_msg": fwd[1].numpy()},
             {"row_msg": want_msgs[0], "col_msg": want_msgs[1]}, {"row_msg": yard_msgs[0], "col_msg": yard_msgs[1]})
    _compare(label, got, want, yard)
    undropped = dg.attention_torch(*[t if t.dtype == torch.bool else t.double() for t in args])
    assert dbc.max_err(fwd[0].numpy(), undropped[0].numpy()) > 1e-3
    # the statistics are those of the call without dropout, and p = 0 gives its messages too
    plain = tgb._attention_forward(lib, d, mask8, None, B, N, H, D, True)
    zero = _attention_forward(lib, d, mask8, None, B, N, H, D, ddc.SEED_ATTN, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(plain[2].cpu(), fwd[2]) and torch.equal(plain[3].cpu(), fwd[3])
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(plain, zero))
    # the ragged call equals the masked uniform call bit for bit (dS outside the prefixes is not touched)
    sizes = dbc.prefix_sizes(B, N).to(torch.int32).to(DEV)
    rag, rag_fwd = _attention_backward(lib, d, g, None, sizes, B, N, H, D, ddc.SEED_ATTN, P, fill=0x3C)
    assert torch.equal(rag_fwd[0], fwd[0]) and torch.equal(rag_fwd[1], fwd[1])
    real = mask[:, None, :].expand(B, H, N)  # a padded query's statistics are never used and differ: (0, 0), (-inf, 0)
    assert torch.equal(rag_fwd[2][real], fwd[2][real]) and torch.equal(rag_fwd[3][real], fwd[3][real])
    keep = mask.numpy()
    pair = np.broadcast_to(keep[:, None, None, :, None] & keep[:, None, None, None, :], got["dS"].shape)
    for name in dbc.ATT_NAMES[1:]:
        assert np.array_equal(got[name], rag[name]), name
    assert np.array_equal(rag["dS"][pair], got["dS"][pair]) and np.all(rag["dS"][~pair] == np.float32(SENTINEL))
    assert not got["dS"][~pair].any()
    # equal inputs and an equal seed give equal bits; p = 0 gives the bits of the backward without dropout
    again, _ = _attention_backward(lib, d, g, mask8, None, B, N, H, D, ddc.SEED_ATTN, P, fill=0xA5)
    off, _ = tgb._attention_backward(lib, d, g, mask8, None, B, N, H, D, 0)
    zero, _ = _attention_backward(lib, d, g, mask8, None, B, N, H, D, ddc.SEED_ATTN, 0.0)
    for name in dbc.ATT_NAMES:
        assert np.array_equal(got[name], again[name]), name
        assert np.array_equal(off[name], zero[name]), name


# ---- lapwarm_dual_edge_scores_backward_dropout -----------------------------------------------------------------

def _edge_backward(lib, d, dS, sizes, B, N, heads, seed, p, fill=0):
    ws, nbytes = tgb._workspace(lib, B, N, heads, fill)
    shapes = {"dW1": (128, 10), "db1": (128,), "dW2": (128, 128), "db2": (128,), "dG": (2 * heads, 128)}
    out = {k: torch.full(s, SENTINEL, device=DEV) for k, s in shapes.items()}
    rc = lib.lapwarm_dual_edge_scores_backward_dropout(
        *[t.data_ptr() for t in d], dS.data_ptr(), _ptr(sizes), *[out[k].data_ptr() for k in dbc.EDGE_NAMES], B, N,
        heads, ws.data_ptr(), nbytes, seed, p, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in out.items()}


def _dropped_edge_autograd(args, dS, mask0, dtype):
    edge = args[0].detach().to(dtype)
    leaves = [t.detach().to(dtype).requires_grad_() for t in args[1:]]
    (ddc.edge_scores_torch(edge, *leaves, mask0) * dS.to(dtype)).sum().backward()
    return dict(zip(dbc.EDGE_NAMES, (t.grad for t in leaves)))


@pytest.mark.parametrize("B,N,sizes", [(1, 17, None), (2, 130, None), (3, 130, (97, 130, 130))],
                         ids=["1x17", "2x130", "sizes_97_130_130"])
def test_edge_scores_backward_with_dropout_against_fp64_autograd(lib, B, N, sizes):
    heads, seed = 4, ddc.SEED_EDGE_BWD
    chunk = lib.lapwarm_dual_backward_chunk()
    assert (B, N) in ddc.EDGE_BWD_SHAPES
    if (B, N) == (2, 130):
        assert B * N * N == 33800 > chunk  # more than one chunk of edges
    if sizes is not None:  # the chunk-crossing case: the second chunk of the ragged walk starts inside an instance
        crossings = dbc.chunk_crossings(sizes, N, chunk)
        assert crossings and all(0 < off < dbc.ragged_wave_tiles(sizes, N)[b] for _, b, off in crossings)
    args, dS = dbc.edge_case(B, N, heads)
    mask0 = ddc.edge_mask(seed, P, B, N)
    if sizes is not None:  # the uniform reference on a dS that is zero outside the prefixes
        keep = dbc.prefix_mask(sizes, N)
        pair = (keep[:, :, None] & keep[:, None, :])[:, None, None].expand_as(dS)
        nan = float("nan")
        dS_ref = torch.where(pair, dS, torch.zeros_like(dS))
        dS_dev = torch.where(pair, dS, torch.full_like(dS, nan))
        edge_dev = torch.where(pair[:, 0, 0, :, :, None], args[0], torch.full_like(args[0], nan))
        sizes_dev = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    else:
        dS_ref, dS_dev, edge_dev, sizes_dev = dS, dS, args[0], None
    want = _dropped_edge_autograd(args, dS_ref, mask0, torch.float64)
    yard = _dropped_edge_autograd(args, dS_ref, mask0, torch.float32)
    d = [edge_dev.to(DEV).contiguous()] + [t.to(DEV).contiguous() for t in args[1:]]
    dS_dev = dS_dev.to(DEV).contiguous()
    label = f"edge backward B={B} N={N} p={P}{'' if sizes is None else f' sizes {sizes}'}"
    got = _edge_backward(lib, d, dS_dev, sizes_dev, B, N, heads, seed, P)
    _compare(label, got, want, yard)
    undropped = dbc.edge_scores_autograd(args, dS_ref)
    assert dbc.max_err(got["dW2"], undropped["dW2"].numpy()) > 1e-3 * float(undropped["dW2"].abs().max())
    again = _edge_backward(lib, d, dS_dev, sizes_dev, B, N, heads, seed, P, fill=0xA5)
    zero = _edge_backward(lib, d, dS_dev, sizes_dev, B, N, heads, seed, 0.0)
    off = tgb._edge_backward(lib, d, dS_dev, sizes_dev, B, N, heads, 0)
    for name in dbc.EDGE_NAMES:
        assert np.array_equal(got[name], again[name]), name
        assert np.array_equal(zero[name], off[name]), name


# ---- the model -------------------------------------------------------------------------------------------------

def _fused_model(cfg, generator_seed):
    model = dg.build_model(cfg).to(DEV)
    model.fused_attention_training = True
    model.fused_dropout = True
    for layer in model.layers:  # the update MLPs' dropouts off: they draw from torch's device generator
        layer.row_update[2].p = layer.col_update[2].p = 0.0
    model.dropout_generator = torch.Generator().manual_seed(generator_seed)
    return model.train()


def _check_model(cfg, inputs, sizes):
    edge, row, col, mask = inputs
    B, N = edge.shape[:2]
    gu, gv = tgb._seeds((B, N), 11)
    fused = _fused_model(cfg, ddc.MODEL_GENERATOR_SEED)
    assert (B, N, fused.heads) in ddc.MODEL_SHAPES and len(fused.layers) == ddc.MODEL_LAYERS
    assert fused.layers[0]._fused_dropout_rates() == (P, P)
    seeds = ddc.layer_seeds(torch.Generator().manual_seed(ddc.MODEL_GENERATOR_SEED), len(fused.layers))
    ref64, ref32 = dg.build_model(cfg, torch.float64), dg.build_model(cfg)
    for m in (ref64, ref32):
        ddc.install_masks(m, seeds, P, B, N)
        m.train()
    want = tgb._model_grads(ref64, edge.double(), row.double(), col.double(), mask, None, gu.double(), gv.double())
    yard = tgb._model_grads(ref32, edge, row, col, mask, None, gu, gv)
    want["u"], yard["u"] = (m(e, r, c, mask)["u"].detach() for m, e, r, c in (
        (ref64, edge.double(), row.double(), col.double()), (ref32, edge, row, col)))
    dev = [t.to(DEV) for t in (edge, row, col)]
    assert fused.layers[0].takes_fused_path(*dev)
    mask_d, sizes_d = None if mask is None else mask.to(DEV), None if sizes is None else sizes.to(DEV)
    got = tgb._model_grads(fused, *dev, mask_d, sizes_d, gu.to(DEV), gv.to(DEV))
    fused.dropout_generator = torch.Generator().manual_seed(ddc.MODEL_GENERATOR_SEED)
    with torch.no_grad():  # training mode without a recorded gradient: the same masks
        got["u"] = (fused(*dev, mask_d) if sizes is None else fused(*dev, mask_d, sizes=sizes_d))["u"].cpu()
    label = f"{cfg} fused dropout p={P}{'' if sizes is None else f' sizes {tuple(sizes.tolist())}'}"
    _compare(label, {k: v.numpy() for k, v in got.items()}, want, yard)


def test_model_outputs_and_gradients_with_fused_dropout_on_the_padded_fixture(lib):
    _check_model("h32_H4_L2", dg.model_inputs("h32_H4_L2@pad"), None)


def test_model_outputs_and_gradients_with_fused_dropout_and_sizes(lib):
    edge, row, col, mask, sizes = tgb._padded_case((5, 17, 12))
    _check_model("h32_H4_L2", (edge, row, col, mask), sizes)


def test_determinism_and_what_the_switch_changes(lib):
    edge, row, col, mask = (t.to(DEV) for t in dg.model_inputs("h32_H4_L2@pad"))
    gu, gv = (t.to(DEV) for t in tgb._seeds(tuple(edge.shape[:2]), 3))
    model = _fused_model("h32_H4_L2", 5)

    def run(generator_seed):
        model.dropout_generator = torch.Generator().manual_seed(generator_seed)
        grads = tgb._model_grads(model, edge, row, col, mask, None, gu, gv)
        model.dropout_generator = torch.Generator().manual_seed(generator_seed)
        with torch.no_grad():
            grads["u"] = model(edge, row, col, mask)["u"].cpu()
        return grads

    a, b, c = run(5), run(5), run(6)
    assert all(torch.equal(a[k], b[k]) for k in a)  # the same generator state: equal bits, gradients included
    assert not torch.equal(a["u"], c["u"])          # another seed: another mask
    # the switch off in training: the fused training forward as it was, and no seed is drawn
    model.fused_dropout = False
    g = torch.Generator().manual_seed(5)
    state = g.get_state()
    model.dropout_generator = g
    with torch.no_grad():
        off = model(edge, row, col, mask)["u"]
        assert torch.equal(g.get_state(), state)
        model.fused_dropout = True
        for layer in model.layers:
            layer.edge_mlp[2].p = layer.dropout.p = 0.0  # on with p = 0: nothing is applied, no seed either
        zero = model(edge, row, col, mask)["u"]
        assert torch.equal(g.get_state(), state)
        for layer in model.layers:
            layer.edge_mlp[2].p = layer.dropout.p = P
        on = model(edge, row, col, mask)["u"]
        assert not torch.equal(g.get_state(), state)
    assert torch.equal(off, zero) and not torch.equal(off.cpu(), on.cpu())
    # eval mode with the switch on: the bits of eval
    model.eval()
    with torch.no_grad():
        eval_on = model(edge, row, col, mask)["u"]
        model.fused_dropout = False
        eval_off = model(edge, row, col, mask)["u"]
    assert torch.equal(eval_on, eval_off)


def test_a_step_with_fused_dropout_stores_no_mask(lib):
    """B = 1, n = 256, hidden 128, 4 layers: the peak of a training step with fused dropout exceeds that of the same
    step without it by less than ONE layer's byte mask of the edge MLP, n^2 * 128 bytes."""
    from gnn.dual_gnn import DualGNN
    n, hidden, layers = 256, 128, 4
    bound = n * n * 128
    torch.manual_seed(0)
    model = DualGNN(hidden_dim=hidden, layers=layers, heads=4, dropout=P).to(DEV).train()
    model.fused_attention_training = True
    model.dropout_generator = torch.Generator().manual_seed(1)
    g = torch.Generator().manual_seed(1)
    edge = (torch.rand((1, n, n, 10), generator=g) * 2.0 - 0.5).to(DEV)
    row, col = torch.randn((1, n, 14), generator=g).to(DEV), torch.randn((1, n, 14), generator=g).to(DEV)

    def peak(on):
        model.fused_dropout = on
        for _ in range(2):  # the first step of either kind warms the allocator
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = model(edge, row, col)
            (out["u"].sum() + out["v_hint"].sum()).backward()
            torch.cuda.synchronize()
            used = torch.cuda.max_memory_allocated() - before
            del out
        return used

    off, on = peak(False), peak(True)
    print(f"peak over the step: without {off / 2**20:.2f} MiB, with fused dropout {on / 2**20:.2f} MiB, "
          f"bound on the difference {bound / 2**20:.0f} MiB")
    assert on - off < bound
