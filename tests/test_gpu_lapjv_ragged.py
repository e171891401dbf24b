"""Cold lapjv of mixed-size and mixed-shape batches on the GPU: `WarmStartPipeline.lapjv_ragged`,
`lapjv_extended_ragged`, `lapjv_extended_many`, `lap.lapjv_many` and the C entry points behind them.

Everything is exact equality: x, y, ret and matched equal, opt bitwise equal.  The yardsticks, in this order: the
reference's own answers (tests/golden/lapjv_extended_cases.npz), the CPU oracle on the numpy-built E with its
ARR iterations, paths and relax steps, and the uniform entries on the instance alone."""
import ctypes as ct

import numpy as np
import pytest

from host_common import pipe, torch_cuda  # noqa: F401
from lapjv_extended_common import ExtendedCases, assert_case, bits, extended_n, solve_with

pytestmark = pytest.mark.gpu

CASES = ExtendedCases()
COUNTERS = ((11, "arr_iters"), (4, "paths"), (6, "scan_steps"))
INF = float("inf")


def _host(o):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


def _uniform(seed, shape):
    return np.random.RandomState(seed).uniform(size=shape)


def _int100(seed, shape):
    return np.random.RandomState(seed).randint(1, 101, size=shape).astype(np.float64)


def _alone(torch, pipe, C, extend_cost, limit):
    """lapjv_extended_batch of one instance: the row of every output."""
    o = _host(pipe.lapjv_extended_batch(torch.from_numpy(np.ascontiguousarray(C)[None]).cuda(), extend_cost, limit))
    return {k: v[0] for k, v in o.items()}


def _assert_equals_alone(label, got, alone, counters=True):
    for key in ("x", "y", "matched", "ret"):
        assert np.array_equal(got[key], alone[key]), (label, key, got[key], alone[key])
    assert bits(got["opt"]) == bits(alone["opt"]), (label, got["opt"], alone["opt"])
    if counters:
        for q, name in COUNTERS:
            assert got["stats"][q] == alone["stats"][q], (label, name, got["stats"][q], alone["stats"][q])


def _assert_equals_oracle(label, C, extend_cost, limit, got):
    from oracle import jv
    opt, x, y, (so,) = solve_with(jv.dense_raw, C, extend_cost, limit)
    st = got["stats"]
    print(f"{label}: n {extended_n(*C.shape, extend_cost, limit)} matched {got['matched']} opt {got['opt']!r} "
          + " ".join(f"{name} {st[q]}/{so[name]}" for q, name in COUNTERS))
    assert got["ret"] == 0, (label, got["ret"], st[12])
    assert np.array_equal(got["x"], x) and np.array_equal(got["y"], y), label
    assert got["matched"] == (x != -1).sum(), label
    assert bits(got["opt"]) == bits(opt), (label, got["opt"], opt)
    for q, name in COUNTERS:
        assert st[q] == so[name], (label, name, st[q], so[name])


def _count_calls(monkeypatch, pipe):
    calls = {"ragged": 0, "batch": 0}
    ragged, batch = pipe.lapjv_extended_ragged, pipe.lapjv_extended_batch

    def count_ragged(*a, **k):
        calls["ragged"] += 1
        return ragged(*a, **k)

    def count_batch(*a, **k):
        calls["batch"] += 1
        return batch(*a, **k)
    monkeypatch.setattr(pipe, "lapjv_extended_ragged", count_ragged)
    monkeypatch.setattr(pipe, "lapjv_extended_batch", count_batch)
    return calls


# --------------------------------------------------------------------------- 1. the reference's fixtures
@pytest.mark.parametrize("extend_cost", (False, True))
def test_all_fixtures_in_one_call(torch_cuda, pipe, monkeypatch, extend_cost):
    cases = [CASES.case(k) for k in range(len(CASES))]
    assert len(cases) == 84
    assert all(extended_n(c["n_rows"], c["n_cols"], c["extend_cost"], c["cost_limit"]) <= 100 for c in cases)
    mine = [c for c in cases if bool(c["extend_cost"]) == extend_cost]
    assert mine
    calls = _count_calls(monkeypatch, pipe)
    out = pipe.lapjv_extended_many([c["C"] for c in mine], extend_cost, [c["cost_limit"] for c in mine])
    assert calls == {"ragged": 1, "batch": 0}
    for c, o in zip(mine, out):
        o = _host(o)
        assert o["ret"] == 0, (c["label"], o["ret"])
        assert o["x"].shape == (c["n_rows"],) and o["y"].shape == (c["n_cols"],)
        assert_case(c, o["opt"], o["x"], o["y"])
        if np.array_equal(o["x"], c["x"]):
            assert o["matched"] == (c["x"] != -1).sum(), c["label"]


# --------------------------------------------------------------------------- 2. every group boundary
# extended n -> (matrix, cost_limit): tall, wide and square shapes, with and without a limit; 65, 127, 129 and 511 are
# odd n with odd n_cols (rows of E on odd element offsets); 1 x k and k x 1
LADDER = {
    1: (lambda: _uniform(1, (1, 1)), INF),
    2: (lambda: _uniform(2, (1, 1)), 2.0),
    63: (lambda: _uniform(3, (1, 63)), INF),
    64: (lambda: _uniform(4, (64, 1)), INF),
    65: (lambda: _uniform(5, (30, 35)), 0.2),
    127: (lambda: _int100(6, (127, 77)), INF),
    128: (lambda: _uniform(7, (128, 128)), INF),
    129: (lambda: _uniform(8, (64, 65)), 0.1),
    255: (lambda: _uniform(9, (100, 255)), INF),
    256: (lambda: _int100(10, (128, 128)), 20.5),
    257: (lambda: _uniform(11, (257, 100)), INF),
    510: (lambda: _uniform(12, (255, 255)), 0.03),
    511: (lambda: _uniform(13, (256, 255)), 0.03),
}


def test_size_ladder_across_every_group_boundary(torch_cuda, pipe, monkeypatch):
    mats = {n: make() for n, (make, _) in LADDER.items()}
    limits = [LADDER[n][1] for n in LADDER]
    assert [extended_n(*mats[n].shape, True, t) for n, t in zip(LADDER, limits)] == list(LADDER)
    alone = {n: _alone(torch_cuda, pipe, mats[n], True, LADDER[n][1]) for n in LADDER}
    calls = _count_calls(monkeypatch, pipe)
    out = pipe.lapjv_extended_many([mats[n] for n in LADDER], True, limits)
    assert calls == {"ragged": 1, "batch": 0}
    for n, o in zip(LADDER, out):
        o = _host(o)
        _assert_equals_oracle(f"n{n}", mats[n], True, LADDER[n][1], o)
        _assert_equals_alone(f"n{n}", o, alone[n])


# --------------------------------------------------------------------------- 3. square ragged cold
def _square_set(cold_cases):
    mats = [cold_cases.case(k)["C"] for k in range(len(cold_cases)) if cold_cases.case(k)["n"] <= 511]
    assert mats
    for n in (64, 65, 256, 257, 511):
        mats += [_uniform(100 + n, (n, n)), _int100(200 + n, (n, n))]
    return [np.ascontiguousarray(C, dtype=np.float64) for C in mats]


def _lapjv_alone(torch, pipe, C):
    x, y, ret, stats = pipe.lapjv_batch(torch.from_numpy(C[None]).cuda())
    return x[0].cpu().numpy(), y[0].cpu().numpy(), int(ret[0]), stats[0].cpu().numpy()


def _assert_rows_equal_alone(mats, out, alone):
    x, y, ret, stats = (t.cpu().numpy() for t in out)
    for b, C in enumerate(mats):
        n = C.shape[0]
        ax, ay, aret, astats = alone[b]
        assert ret[b] == aret, (b, n, ret[b], aret)
        assert np.array_equal(x[b, :n], ax) and np.array_equal(y[b, :n], ay), (b, n)
        assert (x[b, n:] == -1).all() and (y[b, n:] == -1).all(), (b, n)
        for q, name in COUNTERS:
            assert stats[b, q] == astats[q], (b, n, name, stats[b, q], astats[q])
        assert stats[b, 0] == 4  # the cold branch


def test_square_ragged_equals_lapjv_batch_alone_packed_and_padded(torch_cuda, pipe, cold_cases):
    from gnn import ragged_pack
    mats = _square_set(cold_cases)
    alone = [_lapjv_alone(torch_cuda, pipe, C) for C in mats]
    assert all(a[2] == 0 for a in alone)
    packed = pipe.lapjv_ragged(ragged_pack(mats, "cuda:0"))
    assert packed[0].dtype == torch_cuda.int64 and packed[0].shape == (len(mats), 511)
    _assert_rows_equal_alone(mats, packed, alone)
    N = 512  # padded layout, ld = N > every n
    padded = np.full((len(mats), N, N), np.nan)
    for b, C in enumerate(mats):
        padded[b, :C.shape[0], :C.shape[0]] = C
    pack = ragged_pack(padded, "cuda:0", sizes=[C.shape[0] for C in mats])
    assert pack.ld == N
    _assert_rows_equal_alone(mats, pipe.lapjv_ragged(pack), alone)
    one = pipe.lapjv_ragged(ragged_pack(mats[-1:], "cuda:0"), want_stats=True)
    _assert_rows_equal_alone(mats[-1:], one, alone[-1:])
    assert pipe.lapjv_ragged(ragged_pack(mats[:1], "cuda:0"), want_stats=False)[3] is None


def test_square_ragged_of_equal_sizes_reproduces_lapjv_batch(torch_cuda, pipe):
    from gnn import ragged_pack
    torch = torch_cuda
    Cs = np.stack([_uniform(300 + b, (257, 257)) if b % 2 else _int100(300 + b, (257, 257)) for b in range(6)])
    x, y, ret, stats = pipe.lapjv_batch(torch.from_numpy(Cs).cuda())
    rx, ry, rret, rstats = pipe.lapjv_ragged(ragged_pack(list(Cs), "cuda:0"))
    assert torch.equal(rx, x.to(torch.int64)) and torch.equal(ry, y.to(torch.int64)) and torch.equal(rret, ret)
    for q, _ in COUNTERS:
        assert torch.equal(rstats[:, q], stats[:, q]), q


# --------------------------------------------------------------------------- 4. limits below every entry
def test_limit_below_every_entry_next_to_ordinary_instances(torch_cuda, pipe):
    mats = [_uniform(400 + b, shape) + 0.25 for b, shape in enumerate(((33, 58), (40, 40), (70, 21), (90, 90)))]
    limits = [0.2, 0.6, 0.1, INF]  # instances 0 and 2 match nothing
    out = [_host(o) for o in pipe.lapjv_extended_many(mats, True, limits)]
    for b in (0, 2):
        assert out[b]["ret"] == 0 and (out[b]["x"] == -1).all() and (out[b]["y"] == -1).all()
        assert out[b]["matched"] == 0 and bits(out[b]["opt"]) == bits(0.0), out[b]["opt"]  # +0.0, np.sum of nothing
    for b in (1, 3):
        _assert_equals_oracle(f"ordinary{b}", mats[b], True, limits[b], out[b])
        assert out[b]["matched"] > 0


# --------------------------------------------------------------------------- 5. inf and NaN neighbours
def test_inf_and_nan_instances_do_not_touch_their_neighbours(torch_cuda, pipe):
    from lapjv_suite import Suite
    suite = Suite()
    nan_label = min((l for l in suite.nan_labels if suite.matrix(l).shape[0] <= 511),
                    key=lambda l: suite.matrix(l).shape[0])
    sick = [np.array(suite.matrix(l)) for l in ("sparse_square", "inf_unique", nan_label)]
    assert np.isinf(sick[0]).any() and np.isinf(sick[1]).any() and np.isnan(sick[2]).any()
    mats = [_uniform(500, (120, 120)), sick[0], _int100(501, (65, 65)), sick[2], sick[1], _uniform(502, (300, 300))]
    alone = [_alone(torch_cuda, pipe, C, False, INF) for C in mats]
    out = [_host(o) for o in pipe.lapjv_extended_many(mats, False, INF)]
    for b, (o, a) in enumerate(zip(out, alone)):
        assert o["ret"] == a["ret"], (b, o["ret"], a["ret"])
        assert np.array_equal(o["x"], a["x"]) and np.array_equal(o["y"], a["y"]), b
    for b in (0, 2, 5):
        _assert_equals_alone(f"healthy{b}", out[b], alone[b])
        assert out[b]["ret"] == 0 and (out[b]["x"] >= 0).all()


# --------------------------------------------------------------------------- raw calls
def _raw_call_ragged(torch, lib, mats, limits, extend_cost=True, fill=None, stream=None, want_opt=True,
                     want_matched=True, odd=False, descending=False, expect=0):
    """lapwarm_lapjv_extended_ragged with buffers of this test's own.  odd: C starts one double into a 16-byte
    aligned buffer; descending: the instances are stored in reverse order, so that the offsets fall."""
    B = len(mats)
    rows, cols = [C.shape[0] for C in mats], [C.shape[1] for C in mats]
    order = range(B - 1, -1, -1) if descending else range(B)
    offsets, flat, pos = [0] * B, [], 0
    for b in order:
        offsets[b] = pos
        flat.append(np.ascontiguousarray(mats[b], dtype=np.float64).reshape(-1))
        pos += mats[b].size
    buf = torch.empty((pos + 2,), dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    C = buf[1:1 + pos] if odd else buf[:pos]
    C.copy_(torch.from_numpy(np.concatenate(flat)))
    assert C.data_ptr() % 16 == (8 if odd else 0)
    d_off = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    d_rows = torch.tensor(rows, dtype=torch.int32, device="cuda")
    d_cols = torch.tensor(cols, dtype=torch.int32, device="cuda")
    d_lim = torch.tensor(limits, dtype=torch.float64, device="cuda")
    h_rows, h_cols, h_lim = (ct.c_int * B)(*rows), (ct.c_int * B)(*cols), (ct.c_double * B)(*limits)
    nbytes = lib.lapwarm_lapjv_extended_ragged_workspace_bytes(h_rows, h_cols, h_lim, int(extend_cost), B)
    assert nbytes > 0
    R, Q = max(rows), max(cols)
    x = torch.full((B, R), -7, dtype=torch.int32, device="cuda")
    y = torch.full((B, Q), -7, dtype=torch.int32, device="cuda")
    opt = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    matched = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ret = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    torch.cuda.synchronize()
    s = stream.cuda_stream if stream is not None else 0
    rc = lib.lapwarm_lapjv_extended_ragged(
        C.data_ptr(), d_off.data_ptr(), d_rows.data_ptr(), d_cols.data_ptr(), d_lim.data_ptr(), h_rows, h_cols, h_lim,
        0, int(extend_cost), B, R, Q, x.data_ptr(), y.data_ptr(), opt.data_ptr() if want_opt else None,
        matched.data_ptr() if want_matched else None, ret.data_ptr(), None, ws.data_ptr(), nbytes, ct.c_void_p(s))
    assert rc == expect, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(x=x, y=y, opt=opt, matched=matched, ret=ret).items()}


def _raw_set():
    shapes = ((60, 41), (41, 60), (64, 40), (33, 33), (1, 7), (77, 120), (5, 1))
    mats = [_uniform(600 + b, s) for b, s in enumerate(shapes)]
    return mats, [0.05, INF, 0.05, INF, 0.3, INF, 0.9]


def _assert_same(o, base):
    for key in ("x", "y", "matched", "ret"):
        assert np.array_equal(o[key], base[key]), key
    assert np.array_equal(bits(o["opt"]), bits(base["opt"]))


def test_odd_8_byte_offset_and_descending_offsets(torch_cuda, pipe):
    mats, limits = _raw_set()
    base = _raw_call_ragged(torch_cuda, pipe.lib, mats, limits)
    assert (base["ret"] == 0).all()
    _assert_same(_raw_call_ragged(torch_cuda, pipe.lib, mats, limits, odd=True), base)
    _assert_same(_raw_call_ragged(torch_cuda, pipe.lib, mats, limits, descending=True), base)
    _assert_same(_raw_call_ragged(torch_cuda, pipe.lib, mats, limits, odd=True, descending=True), base)
    from oracle import jv
    for b, (C, t) in enumerate(zip(mats, limits)):
        opt, x, y, _ = solve_with(jv.dense_raw, C, True, t)
        r, c = C.shape
        assert np.array_equal(base["x"][b, :r], x) and np.array_equal(base["y"][b, :c], y), b
        assert (base["x"][b, r:] == -1).all() and (base["y"][b, c:] == -1).all(), b
        assert bits(base["opt"][b]) == bits(opt) and base["matched"][b] == (x != -1).sum(), b


def test_poisoned_workspace_on_a_side_stream_and_null_outputs(torch_cuda, pipe):
    torch = torch_cuda
    mats, limits = _raw_set()
    base = _raw_call_ragged(torch, pipe.lib, mats, limits, fill=0)
    o = _raw_call_ragged(torch, pipe.lib, mats, limits, fill=0xFF, stream=torch.cuda.Stream())
    _assert_same(o, base)
    for want_opt, want_matched in ((False, True), (True, False), (False, False)):
        o = _raw_call_ragged(torch, pipe.lib, mats, limits, fill=0xFF, want_opt=want_opt, want_matched=want_matched)
        assert np.array_equal(o["x"], base["x"]) and np.array_equal(o["y"], base["y"]) and (o["ret"] == 0).all()
        assert np.array_equal(bits(o["opt"]), bits(base["opt"])) if want_opt else (o["opt"] == -7.0).all()
        assert np.array_equal(o["matched"], base["matched"]) if want_matched else (o["matched"] == -7).all()


# --------------------------------------------------------------------------- 8. routing
def test_routing_of_an_instance_outside_the_class(torch_cuda, pipe, monkeypatch):
    mats = [_uniform(700, (50, 70)), _uniform(701, (300, 300)), _uniform(702, (255, 256)), _int100(703, (20, 20))]
    limits = [0.1, 0.02, 0.03, INF]  # instance 1: n = 600
    assert not pipe.lapjv_ragged_eligible(600) and pipe.lapjv_ragged_eligible(511)
    alone = [_alone(torch_cuda, pipe, C, True, t) for C, t in zip(mats, limits)]
    calls = _count_calls(monkeypatch, pipe)
    out = pipe.lapjv_extended_many(mats, True, limits)
    assert calls == {"ragged": 1, "batch": 1}
    for b, o in enumerate(out):
        _assert_equals_alone(f"routing{b}", _host(o), alone[b])
    _raw_call_ragged(torch_cuda, pipe.lib, mats, limits, expect=-6)


# --------------------------------------------------------------------------- 9. the drop-in
def test_lapjv_many_equals_lapjv_extended_per_instance(torch_cuda):
    import lap
    mats = [_uniform(800, (40, 40)), _int100(801, (31, 31)), _uniform(802, (100, 100)), _uniform(803, (300, 300))]
    for extend_cost, limits in ((False, INF), (False, [0.1, 30.5, INF, 0.02]), (True, 0.05)):
        each = limits if isinstance(limits, list) else [limits] * len(mats)
        many = lap.lapjv_many(mats, extend_cost, limits)
        pairs = lap.lapjv_many(mats, extend_cost, limits, return_cost=False)
        for C, t, (opt, x, y), (x2, y2) in zip(mats, each, many, pairs):
            ropt, rx, ry = lap.lapjv_extended(C, extend_cost, t)
            assert type(opt) is type(ropt) and bits(opt) == bits(ropt), (opt, ropt)
            assert x.dtype == rx.dtype == np.int32 and y.dtype == ry.dtype == np.int32
            assert np.array_equal(x, rx) and np.array_equal(y, ry)
            assert np.array_equal(x2, rx) and np.array_equal(y2, ry) and x2.dtype == np.int32
    rect = [_uniform(810, (20, 35)), _uniform(811, (35, 20)), _uniform(812, (1, 9))]
    for (opt, x, y), C in zip(lap.lapjv_many(rect, extend_cost=True), rect):
        ropt, rx, ry = lap.lapjv_extended(C, extend_cost=True)
        assert bits(opt) == bits(ropt) and np.array_equal(x, rx) and np.array_equal(y, ry)
