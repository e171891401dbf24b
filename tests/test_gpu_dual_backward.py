"""The backward of DualGNN's fused attention on the MI355X: lapwarm_dual_attention_backward and
lapwarm_dual_edge_scores_backward against fp64 autograd of dual_gnn_common.attention_torch / edge_scores_torch, the
forward with statistics against the forward without, and DualGNN with fused_attention_training against the fp64
plain-path model on the CPU.

Tolerance, per output: refine_backward_common.tolerance, 4 x the max-abs error of PyTorch-CPU float32 autograd of
the same formulation against the fp64 reference, or 1e-6 * max(1, max|ref|) if that is larger.

Beside the small shapes, cases that reach the later trips of the loops: more partials of dkb than the reducing block
has threads, three chunks of edges (a middle chunk only adds to the running sums), a ragged walk whose chunks start
inside an instance and end past the sizes, empty instances, several key tiles times several column chunks, and a
model step across a chunk.  Each of them asserts that precondition from lapwarm_dual_backward_chunk() and the tile
arithmetic of dual_backward_common before it runs; the figures of one run are in profiles/dual_gnn_backward.md."""
import ctypes as ct

import numpy as np
import pytest
import torch

import dual_backward_common as dbc
import dual_gnn_common as dg
from host_common import device_lib as lib  # noqa: F401
from refine_backward_common import tolerance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = float.fromhex("0x1.5p+100")


def _stream():
    return ct.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _workspace(lib, B, N, H, fill):
    nbytes = lib.lapwarm_dual_backward_workspace_bytes(B, N, H)
    assert nbytes > 0
    return torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV), nbytes


def _compare(label, got, want, yard):
    """got: name -> device result; want: fp64 reference; yard: float32 CPU autograd.  Prints every figure first."""
    bad = []
    for name, ref in want.items():
        ref = ref.numpy() if isinstance(ref, torch.Tensor) else ref
        err32 = dbc.max_err(yard[name].numpy(), ref)
        tol = tolerance(err32, ref)
        err = dbc.max_err(got[name], ref)
        print(f"{label} {name}: device {err:.3e}, torch fp32 {err32:.3e}, tolerance {tol:.3e}")
        assert np.isfinite(got[name]).all(), (label, name)
        if not err <= tol:
            bad.append((name, err, tol))
    assert not bad, (label, bad)


# ---- lapwarm_dual_attention_backward ---------------------------------------------------------------------------

def _attention_forward(lib, d, mask8, sizes, B, N, H, D, stats):
    """d: scores, a_row, c_row, a_col, c_col, kbias, row_val, col_val on the device -> row_msg, col_msg[, stats]"""
    row_msg, col_msg = (torch.full((B, N, H * D), SENTINEL, device=DEV) for _ in range(2))
    head = [t.data_ptr() for t in d[:6]]
    vals = [d[6].data_ptr(), d[7].data_ptr(), row_msg.data_ptr(), col_msg.data_ptr()]
    if not stats:
        if sizes is not None:
            rc = lib.lapwarm_dual_attention_ragged(*head, sizes.data_ptr(), *vals, B, N, H, D, _stream())
        else:
            rc = lib.lapwarm_dual_attention(*head, _ptr(mask8), *vals, B, N, H, D, _stream())
        assert rc == 0
        return row_msg, col_msg
    rs, cs = (torch.full((B, H, N, 2), SENTINEL, device=DEV) for _ in range(2))
    if sizes is not None:
        rc = lib.lapwarm_dual_attention_stats_ragged(*head, sizes.data_ptr(), *vals, rs.data_ptr(), cs.data_ptr(), B, N,
                                                     H, D, _stream())
    else:
        rc = lib.lapwarm_dual_attention_stats(*head, _ptr(mask8), *vals, rs.data_ptr(), cs.data_ptr(), B, N, H, D,
                                              _stream())
    assert rc == 0
    return row_msg, col_msg, rs, cs


def _attention_backward(lib, d, g, mask8, sizes, B, N, H, D, fill):
    """-> name -> NumPy result, and the forward's messages; the workspace and dS start filled with `fill` bytes /
    the sentinel."""
    row_msg, col_msg, rs, cs = _attention_forward(lib, d, mask8, sizes, B, N, H, D, True)
    ws, nbytes = _workspace(lib, B, N, H, fill)
    out = {"dS": torch.full((B, 2, H, N, N), SENTINEL, device=DEV)}
    for name in ("da_row", "dc_row", "da_col", "dc_col"):
        out[name] = torch.full((B, H, N), SENTINEL, device=DEV)
    out["dkb"] = torch.full((2 * H,), SENTINEL, device=DEV)
    out["d_row_val"], out["d_col_val"] = (torch.full((B, N, H * D), SENTINEL, device=DEV) for _ in range(2))
    rc = lib.lapwarm_dual_attention_backward(
        *[t.data_ptr() for t in d[:6]], _ptr(mask8), _ptr(sizes), d[6].data_ptr(), d[7].data_ptr(), row_msg.data_ptr(),
        col_msg.data_ptr(), rs.data_ptr(), cs.data_ptr(), g[0].data_ptr(), g[1].data_ptr(),
        *[out[name].data_ptr() for name in dbc.ATT_NAMES], B, N, H, D, ws.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in out.items()}, (row_msg.cpu(), col_msg.cpu())


def _check_attention(lib, B, N, H, D, mask_kind, scale=1.0, sizes=None):
    """sizes (with mask_kind prefix): what the device gets as sizes, in place of prefix_sizes(B, N); the mask is
    their prefix mask, a size outside 1..N an empty instance."""
    args, grads = dbc.attention_case(B, N, H, D, mask_kind, scale, sizes=sizes)
    mask = args[6]
    want = dbc.attention_autograd(args, grads)
    yard = dbc.attention_autograd(args, grads, torch.float32)
    d = [t.to(DEV).contiguous() for t in args[:6] + args[7:]]
    g = [t.to(DEV).contiguous() for t in grads]
    mask8 = None if mask is None else mask.to(torch.uint8).to(DEV).contiguous()
    label = f"B={B} N={N} H={H} D={D} {mask_kind}{'' if sizes is None else ' ' + str(tuple(sizes))} x{scale:g}"
    got, msgs = _attention_backward(lib, d, g, mask8, None, B, N, H, D, 0)
    _compare(label, got, {k: v for k, v in want.items()}, yard)
    # the forward with statistics gives the bits of the forward without
    plain = _attention_forward(lib, d, mask8, None, B, N, H, D, False)
    torch.cuda.synchronize()
    assert torch.equal(plain[0].cpu(), msgs[0]) and torch.equal(plain[1].cpu(), msgs[1])
    # a reused, dirtied workspace: the same bits
    again, _ = _attention_backward(lib, d, g, mask8, None, B, N, H, D, 0xA5)
    for name in dbc.ATT_NAMES:
        assert np.array_equal(got[name], again[name]), (label, name)
    if mask is not None:
        keep = mask.numpy()
        pair = np.broadcast_to(keep[:, None, None, :, None] & keep[:, None, None, None, :], got["dS"].shape)
        assert not got["dS"][~pair].any()
        node = np.broadcast_to(keep[:, None, :], got["da_row"].shape)
        for name in ("da_row", "dc_row", "da_col", "dc_col"):
            assert not got[name][~node].any(), name
        assert not got["d_row_val"][~keep].any() and not got["d_col_val"][~keep].any()
    if mask_kind == "prefix":  # sizes: the bits of the prefix mask, and dS outside the prefixes is not touched
        sizes = (dbc.prefix_sizes(B, N) if sizes is None else torch.tensor(sizes)).to(torch.int32).to(DEV)
        rag, rag_msgs = _attention_backward(lib, d, g, None, sizes, B, N, H, D, 0x3C)
        assert torch.equal(rag_msgs[0], msgs[0]) and torch.equal(rag_msgs[1], msgs[1])
        for name in dbc.ATT_NAMES[1:]:
            assert np.array_equal(got[name], rag[name]), (label, name)
        assert np.array_equal(rag["dS"][pair], got["dS"][pair])
        assert np.all(rag["dS"][~pair] == np.float32(SENTINEL))
        # sizes take precedence: a mask passed with them, here one that is not their prefix mask, changes no bit
        other = dbc.attention_case(B, N, H, D, "scattered", seed=1)[0][6]
        assert N == 1 or not torch.equal(other, mask)  # one node: both masks are all ones
        both, _ = _attention_backward(lib, d, g, other.to(torch.uint8).to(DEV).contiguous(), sizes, B, N, H, D, 0x3C)
        for name in dbc.ATT_NAMES:
            assert np.array_equal(rag[name], both[name]), (label, name, "sizes and a mask")


MASKS = ("none", "prefix", "scattered", "one_empty")


@pytest.mark.parametrize("D", [3, 16, 32])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 65, 130])
def test_attention_backward_around_the_query_and_key_tiles_under_every_mask(lib, N, D):
    for mask_kind in MASKS:
        _check_attention(lib, 2, N, 2, D, mask_kind)


@pytest.mark.parametrize("H,D", [(1, 160), (1, 8), (3, 8), (8, 8)])
def test_attention_backward_above_the_column_chunk_and_over_the_head_counts(lib, H, D):
    for mask_kind in ("none", "prefix"):
        _check_attention(lib, 2, 33, H, D, mask_kind)


def test_attention_backward_with_logits_scaled_by_100_is_finite(lib):
    for mask_kind in ("none", "scattered"):
        _check_attention(lib, 2, 65, 2, 16, mask_kind, scale=100.0)


KBIAS_BLOCK = 256  # threads of dual_attention_bwd_kbias_kernel; each sums the partials i, i + 256, ...
QUERY_TILE = 16    # queries per workgroup of the query-major kernel: one fp64 partial of dkb each


@pytest.mark.parametrize("B", [128, 129])
def test_attention_backward_sums_the_partials_of_dkb_past_one_trip_of_its_block(lib, B):
    """B * ceil(17 / 16) partials per (direction, head): 256, one trip that fills the block, and 258, where threads
    0 and 1 make a second trip and decode (instance 128, tiles 0 and 1).  Tile 1 holds one query."""
    N, H, D = 17, 2, 3
    count = B * -(-N // QUERY_TILE)
    assert count == (KBIAS_BLOCK if B == 128 else KBIAS_BLOCK + 2), count
    for mask_kind in ("none", "prefix"):
        _check_attention(lib, B, N, H, D, mask_kind)


def test_attention_backward_with_empty_and_out_of_range_sizes(lib):
    """sizes (33, 0, 34, 20) at N = 33: instances 1 and 2 are empty.  Against the prefix mask of (33, 0, 0, 20);
    _check_attention asserts exact zeros in da, dc, dval outside the prefixes, the sentinel in dS outside them (the
    whole planes of instances 1 and 2) and that a scattered mask passed with the sizes changes no bit."""
    N, sizes = 33, (33, 0, 34, 20)
    keep = dbc.prefix_mask(sizes, N)
    assert [int(k.sum()) for k in keep] == [33, 0, 0, 20]
    assert any(s < 1 for s in sizes) and any(s > N for s in sizes)
    _check_attention(lib, len(sizes), N, 2, 8, "prefix", sizes=sizes)


@pytest.mark.parametrize("B,N,D", [(1, 65, 130), (2, 130, 160)])
def test_attention_backward_over_several_key_tiles_and_column_chunks_at_once(lib, B, N, D):
    assert N > 64 and D > 128  # more than one key tile of 64 and more than one pass of 128 columns
    for mask_kind in ("none", "scattered"):
        _check_attention(lib, B, N, 1, D, mask_kind)


# ---- lapwarm_dual_edge_scores_backward -------------------------------------------------------------------------

def _edge_backward(lib, d, dS, sizes, B, N, heads, fill):
    ws, nbytes = _workspace(lib, B, N, heads, fill)
    shapes = {"dW1": (128, 10), "db1": (128,), "dW2": (128, 128), "db2": (128,), "dG": (2 * heads, 128)}
    out = {k: torch.full(s, SENTINEL, device=DEV) for k, s in shapes.items()}
    rc = lib.lapwarm_dual_edge_scores_backward(*[t.data_ptr() for t in d], dS.data_ptr(), _ptr(sizes),
                                               *[out[k].data_ptr() for k in dbc.EDGE_NAMES], B, N, heads,
                                               ws.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_edge(lib, B, N, heads, ragged=True, sizes=None, all_n=False):
    """sizes: what the ragged call gets in place of prefix_sizes(B, N), a size outside 1..N an empty instance;
    all_n: also the call with every size N against the reference of the uniform call."""
    args, dS = dbc.edge_case(B, N, heads)
    want = dbc.edge_scores_autograd(args, dS)
    yard = dbc.edge_scores_autograd(args, dS, torch.float32)
    d = [t.to(DEV).contiguous() for t in args]
    label = f"B={B} N={N} heads={heads}"
    got = _edge_backward(lib, d, dS.to(DEV).contiguous(), None, B, N, heads, 0)
    _compare(label, got, want, yard)
    again = _edge_backward(lib, d, dS.to(DEV).contiguous(), None, B, N, heads, 0xA5)
    for name in dbc.EDGE_NAMES:
        assert np.array_equal(got[name], again[name]), (label, name)
    if all_n:
        full = _edge_backward(lib, d, dS.to(DEV).contiguous(), torch.full((B,), N, dtype=torch.int32, device=DEV), B, N,
                              heads, 0x3C)
        _compare(label + " sizes all N", full, want, yard)
    if not ragged:
        return
    # sizes: the uniform call on a dS that is zero outside the prefixes; NaN outside the prefixes is never read.  The
    # ragged walk numbers its wave tiles row by row, so the same terms are summed in another grouping: equal within
    # the tolerance, not in the bits.
    sizes = dbc.prefix_sizes(B, N) if sizes is None else torch.tensor(sizes)
    label += f" sizes {tuple(sizes.tolist())}" if B <= 8 else " sizes"
    keep = dbc.prefix_mask(sizes, N)
    pair = (keep[:, :, None] & keep[:, None, :])[:, None, None].expand_as(dS)
    zeroed = torch.where(pair, dS, torch.zeros_like(dS))
    want0, yard0 = want, yard  # every size N: nothing is zeroed and the references above hold
    if not bool(pair.all()):
        want0 = dbc.edge_scores_autograd(args, zeroed)
        yard0 = dbc.edge_scores_autograd(args, zeroed, torch.float32)
    uniform = _edge_backward(lib, d, zeroed.to(DEV).contiguous(), None, B, N, heads, 0)
    nan = float("nan")
    edge_nan = torch.where(pair[:, 0, 0, :, :, None], args[0], torch.full_like(args[0], nan))
    d_nan = [edge_nan.to(DEV).contiguous()] + d[1:]
    dS_nan = torch.where(pair, dS, torch.full_like(dS, nan)).to(DEV).contiguous()
    rag = _edge_backward(lib, d_nan, dS_nan, sizes.to(torch.int32).to(DEV), B, N, heads, 0x3C)
    _compare(label, rag, want0, yard0)
    _compare(label + ": uniform, zeroed", uniform, want0, yard0)
    again = _edge_backward(lib, d_nan, dS_nan, sizes.to(torch.int32).to(DEV), B, N, heads, 0xA5)
    for name in dbc.EDGE_NAMES:
        assert np.array_equal(rag[name], again[name]), (label, name)


@pytest.mark.parametrize("heads", [1, 3, 4, 8])
@pytest.mark.parametrize("B,N", [(1, 3), (1, 17), (2, 130)])
def test_edge_scores_backward_against_fp64_autograd(lib, B, N, heads):
    _check_edge(lib, B, N, heads)


def test_edge_scores_backward_across_a_chunk_boundary_by_less_than_a_tile(lib):
    chunk = lib.lapwarm_dual_backward_chunk()
    found = None
    for N in range(3, 12):
        B = chunk // (N * N) + 1
        if 0 < B * N * N - chunk <= 16:
            found = (B, N)
            break
    assert found, chunk
    print(f"chunk {chunk}: B={found[0]} N={found[1]}, {found[0] * found[1] ** 2 - chunk} edges past it")
    _check_edge(lib, found[0], found[1], 4, ragged=False)


def _chunks_of(lib, tiles):
    per = lib.lapwarm_dual_backward_chunk() // dbc.WAVE_EDGES
    return -(-tiles // per)


def _three_chunk_shape(lib):
    """The smallest N whose N^2 edges reach into a third chunk, in the uniform and in the ragged numbering: the
    middle chunk neither starts nor ends the running sums."""
    chunk = lib.lapwarm_dual_backward_chunk()
    N = next(n for n in range(1, 2049) if n * n > 2 * chunk)
    uniform, ragged = -(-N * N // dbc.WAVE_EDGES), dbc.ragged_wave_tiles((N,), N)[0]
    found = f"chunk {chunk}: N={N}, {N * N - 2 * chunk} edges into the third chunk, {uniform} uniform tiles in " \
            f"{_chunks_of(lib, uniform)} chunks, {ragged} ragged tiles in {_chunks_of(lib, ragged)} chunks"
    print(found)
    assert _chunks_of(lib, uniform) >= 3 and _chunks_of(lib, ragged) >= 3, found
    return N


def test_edge_scores_backward_over_three_chunks_uniform_and_ragged(lib):
    N = _three_chunk_shape(lib)
    _check_edge(lib, 1, N, 4, sizes=(N,))  # the ragged walk has rows in all three chunks too


def test_edge_scores_backward_of_a_gradient_on_the_chunk_boundaries_alone(lib):
    """dS is zero but on the wave tile before and the wave tile after every chunk boundary, of the uniform and of
    the ragged numbering: a boundary tile dropped, doubled or shifted is the whole signal."""
    N, heads = _three_chunk_shape(lib), 4
    per = lib.lapwarm_dual_backward_chunk() // dbc.WAVE_EDGES
    edges = []
    for k in range(1, _chunks_of(lib, -(-N * N // dbc.WAVE_EDGES))):
        edges += dbc.uniform_tile_edges(1, N, k * per - 1) + dbc.uniform_tile_edges(1, N, k * per)
    for k in range(1, _chunks_of(lib, dbc.ragged_wave_tiles((N,), N)[0])):
        edges += dbc.ragged_tile_edges((N,), N, k * per - 1) + dbc.ragged_tile_edges((N,), N, k * per)
    assert len(edges) >= 4 * 16 and len(set(edges)) == len(edges), len(edges)
    args, dS = dbc.edge_case(1, N, heads)
    probe = dbc.probe_gradient(dS, edges)
    assert int(probe[0, 0, 0].count_nonzero()) == len(edges)
    want = dbc.edge_scores_autograd(args, probe)
    yard = dbc.edge_scores_autograd(args, probe, torch.float32)
    d = [t.to(DEV).contiguous() for t in args]
    label = f"B=1 N={N} heads={heads} probe of {len(edges)} edges"
    uniform = _edge_backward(lib, d, probe.to(DEV).contiguous(), None, 1, N, heads, 0)
    _compare(label, uniform, want, yard)
    rag = _edge_backward(lib, d, probe.to(DEV).contiguous(), torch.tensor([N], dtype=torch.int32, device=DEV), 1, N,
                         heads, 0x3C)
    _compare(label + " sizes", rag, want, yard)


@pytest.mark.parametrize("heads", [1, 4])
def test_edge_scores_backward_ragged_walk_across_chunk_boundaries_with_empty_instances(lib, heads):
    """sizes (130, 0, 97, 130, 131, 130): two chunk starts fall inside an instance (the branch of the walk whose
    first tile is not the instance's first), the sizes end inside the third chunk (eb_chunk_rows clamps it), the
    fourth has no row, and 0 and 131 are the two kinds of empty instance."""
    N, sizes = 130, (130, 0, 97, 130, 131, 130)
    B = len(sizes)
    counts = dbc.ragged_wave_tiles(sizes, N)
    per = lib.lapwarm_dual_backward_chunk() // dbc.WAVE_EDGES
    crossings = dbc.chunk_crossings(sizes, N, per * dbc.WAVE_EDGES)
    padded = B * dbc.ragged_wave_tiles((N,), N)[0]
    found = f"{counts} tiles, chunks of {per}: crossings {crossings}, {sum(counts)} of {padded} padded tiles"
    print(found)
    assert len(crossings) >= 2 and all(0 < off < counts[b] for _, b, off in crossings), found
    assert sum(counts) % per and _chunks_of(lib, sum(counts)) < _chunks_of(lib, padded), found
    assert any(s < 1 for s in sizes) and any(s > N for s in sizes) and counts.count(0) == 2, found
    _check_edge(lib, B, N, heads, sizes=sizes, all_n=True)


# ---- the model -------------------------------------------------------------------------------------------------

def _seeds(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def _model_grads(model, edge, row, col, mask, sizes, gu, gv):
    """-> name -> gradient (CPU tensors) of sum(u * gu) + sum(v_hint * gv) for every parameter, row_feat, col_feat"""
    model.zero_grad(set_to_none=True)
    row, col = row.detach().clone().requires_grad_(), col.detach().clone().requires_grad_()
    out = model(edge, row, col, mask) if sizes is None else model(edge, row, col, mask, sizes=sizes)
    assert out["u"].requires_grad
    ((out["u"] * gu).sum() + (out["v_hint"] * gv).sum()).backward()
    grads = {name: p.grad.detach().cpu() for name, p in model.named_parameters()}
    grads["row_feat"], grads["col_feat"] = row.grad.detach().cpu(), col.grad.detach().cpu()
    return grads


def _padded_case(sizes=(5, 17, 12)):
    """A padded batch of the sizes: features of random instances, zero outside the prefixes."""
    rs = np.random.RandomState(5)
    B, N = len(sizes), max(sizes)
    edge, row, col = np.zeros((B, N, N, 10), np.float32), np.zeros((B, N, 14), np.float32), np.zeros((B, N, 14), np.float32)
    for b, n in enumerate(sizes):
        e, r, c = dg.features_numpy(rs.uniform(0.0, 1.0, (n, n)))
        edge[b, :n, :n], row[b, :n], col[b, :n] = e, r, c
    mask = torch.arange(N)[None, :] < torch.tensor(sizes)[:, None]
    return torch.from_numpy(edge), torch.from_numpy(row), torch.from_numpy(col), mask, torch.tensor(sizes, dtype=torch.int32)


def _check_model(cfg, inputs, sizes, train):
    edge, row, col, mask = inputs
    gu, gv = _seeds(tuple(edge.shape[:2]), 11)
    ref64 = dg.build_model(cfg, torch.float64)
    ref32 = dg.build_model(cfg)
    fused = dg.build_model(cfg).to(DEV)
    fused.fused_attention_training = True
    for m in (ref64, ref32, fused):
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        m.train(train)
    want = _model_grads(ref64, edge.double(), row.double(), col.double(), mask, None, gu.double(), gv.double())
    yard = _model_grads(ref32, edge, row, col, mask, None, gu, gv)
    edge_d = edge.to(DEV)
    assert fused.layers[0].takes_fused_path(edge_d, row.to(DEV), col.to(DEV))
    got = _model_grads(fused, edge_d, row.to(DEV), col.to(DEV), None if mask is None else mask.to(DEV),
                       None if sizes is None else sizes.to(DEV), gu.to(DEV), gv.to(DEV))
    label = f"{cfg} {'train' if train else 'eval'}{'' if sizes is None else f' sizes {tuple(sizes.tolist())}'}"
    _compare(label, {k: v.numpy() for k, v in got.items()}, want, yard)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("label", ["h32_H4_L2@uniform_n17", "h128_H4_L1@uniform_n65", "h64_H8_L1@pad"])
def test_model_gradients_on_the_fused_path_match_the_fp64_plain_path(lib, label, train):
    _check_model(label.split("@")[0], dg.model_inputs(label), None, train)


@pytest.mark.parametrize("train", [False, True])
def test_model_gradients_with_sizes_on_a_padded_batch(lib, train):
    edge, row, col, mask, sizes = _padded_case()
    _check_model("h32_H4_L2", (edge, row, col, mask), sizes, train)


def test_model_gradients_with_sizes_on_a_padded_batch_whose_edge_backward_crosses_a_chunk(lib):
    """sizes (97, 130, 130): the padded edges take two chunks in either numbering, and the second chunk of the ragged
    walk starts inside the third instance.  Every layer's backward runs the wrappers' workspace and the
    zero-initialised dS under sizes in that regime."""
    sizes = (97, 130, 130)
    N, chunk = max(sizes), lib.lapwarm_dual_backward_chunk()
    counts = dbc.ragged_wave_tiles(sizes, N)
    crossings = dbc.chunk_crossings(sizes, N, chunk)
    found = f"chunk {chunk}: {len(sizes) * N * N} padded edges, {counts} tiles, crossings {crossings}"
    print(found)
    assert len(sizes) * N * N > chunk and _chunks_of(lib, sum(counts)) >= 2, found
    assert crossings and all(0 < off < counts[b] for _, b, off in crossings), found
    edge, row, col, mask, sizes = _padded_case(sizes)
    _check_model("h32_H4_L2", (edge, row, col, mask), sizes, False)


def test_one_training_step_with_dropout_gives_finite_gradients(lib):
    model = dg.build_model("h32_H4_L2").to(DEV)
    model.fused_attention_training = True
    model.train()
    edge, row, col, mask = (t.to(DEV) for t in dg.model_inputs("h32_H4_L2@pad"))
    torch.manual_seed(0)
    a = model(edge, row, col, mask)["u"]
    b = model(edge, row, col, mask)["u"]
    assert not torch.equal(a, b)  # the update MLPs' dropout is active
    gu, gv = _seeds(tuple(edge.shape[:2]), 3)
    grads = _model_grads(model, edge, row, col, mask, None, gu.to(DEV), gv.to(DEV))
    assert all(torch.isfinite(g).all() for g in grads.values())
    assert any(g.abs().max() > 0 for k, g in grads.items() if "edge_mlp.0" in k)


def test_the_eval_forward_without_gradients_does_not_depend_on_the_switch(lib):
    model = dg.build_model("h32_H4_L2").to(DEV)
    edge, row, col, mask = (t.to(DEV) for t in dg.model_inputs("h32_H4_L2@pad"))
    with torch.no_grad():
        off = model(edge, row, col, mask)
        model.fused_attention_training = True
        assert model.layers[0].takes_fused_path(edge, row, col)
        on = model(edge, row, col, mask)
    assert torch.equal(off["u"], on["u"]) and torch.equal(off["v_hint"], on["v_hint"])
    assert not on["u"].requires_grad


def test_a_fused_training_step_keeps_no_edge_embedding_and_the_plain_path_does(lib):
    """B = 1, n = 256, hidden 128, 4 layers, 4 heads: one edge embedding per layer is layers * n^2 * hidden * 4 bytes
    = 128 MiB, which the plain path saves for its backward and the fused path never forms."""
    from gnn.dual_gnn import DualGNN
    n, hidden, layers = 256, 128, 4
    bound = layers * n * n * hidden * 4
    torch.manual_seed(0)
    model = DualGNN(hidden_dim=hidden, layers=layers, heads=4, dropout=0.0).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    edge = (torch.rand((1, n, n, 10), generator=g) * 2.0 - 0.5).to(DEV)
    row, col = torch.randn((1, n, 14), generator=g).to(DEV), torch.randn((1, n, 14), generator=g).to(DEV)

    def peak(on):
        model.fused_attention_training = on
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = model(edge, row, col)
        (out["u"].sum() + out["v_hint"].sum()).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    fused, plain = peak(True), peak(False)
    print(f"peak over the step: fused {fused / 2**20:.1f} MiB, plain {plain / 2**20:.1f} MiB, bound {bound / 2**20:.0f} MiB")
    assert fused < bound <= plain
