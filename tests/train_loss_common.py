"""Reader of tests/golden/train_loss_cases.npz, the input recipes of the training-loss cases and a NumPy
restatement of the OneGNN training loss (shared by tests/golden/make_train_loss.py, test_train_loss_fixtures.py,
test_gpu_train_loss.py and test_gpu_train_loss_large.py).

The cases above n = 257 are never stored: large_case() regenerates them from np.random.default_rng(seed) with
the fixed seeds of LARGE_SPECS, and tests/golden/train_loss_large_ref.npz holds, for two of them, what the
reference computed and a CRC32 of the input bytes.

The restatement is written from the definition of the loss, not from the reference's code.  Per instance with
n_b valid rows and columns (a prefix of the padded matrix), all terms float32:

    v_j = min_i (C_ij - u_i), a_j the LOWEST row attaining it
    h_ij = max((u_i + v_j) - C_ij, 0),  reduced_ij = (C_ij - u_i) - v_j
    greedy: rows in STABLE ascending order of min_j reduced_ij; each takes its cheapest unused column, the
            LOWEST one among equals; primal_upper = the costs summed over rows 0..n_b-1 in float64, rounded once
    cnt_i = #{j: a_j = i}, R_i = #{j: h_ij > 0}, K_j = #{i: h_ij > 0}
    g_i = (1/B) [ w0 (cnt_i - 1) + w1 (R_i - sum_{a_j = i} K_j) / n_b^2 + w2 2 (u_i - t_i) / n_b ]
"""
import json
import zlib
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "train_loss_cases.npz"
LARGE_REF = Path(__file__).resolve().parent / "golden" / "train_loss_large_ref.npz"
WEIGHTS = (1.0, 1.0, 0.1)
F32_EPS = 2.0 ** -24  # unit roundoff of float32
GRID_SCALE = np.float32(0.7310586)  # no power of two: the products below use the whole mantissa


def cost_from_grid(q):
    """float32 costs in [0, 0.74) from 12-bit integers: the large fixtures store q (2 bytes, compressible)."""
    return (q.astype(np.float32) / np.float32(4096)) * GRID_SCALE


def grid_from_cost(cost):
    q = np.rint(cost.astype(np.float64) / float(GRID_SCALE) * 4096).astype(np.uint16)
    assert np.array_equal(cost_from_grid(q).view(np.int32), np.ascontiguousarray(cost).view(np.int32))
    return q


def uniform_case(rng, B, n, sizes):
    """Costs uniform in [0, 1), u_pred = u_target + noise with |u| up to 4: u + v then rounds more coarsely than
    C, which leaves the positive hinge residue the loss has to reproduce.  From n = 257 the costs are
    cost_from_grid(q) of 12-bit integers q, and q is what the golden file stores, so that it stays small.
    Finite rubbish in the padding, which no valid entry may depend on."""
    if n < 257:
        cost = rng.random(size=(B, n, n), dtype=np.float32)
    else:
        cost = cost_from_grid(rng.integers(0, 1 << 12, size=(B, n, n)).astype(np.uint16))
    u_target = rng.uniform(-4.0, 4.0, size=(B, n)).astype(np.float32)
    u_pred = (u_target + 0.05 * rng.standard_normal((B, n))).astype(np.float32)
    return pad(cost, u_pred, u_target, sizes)


def integer_case(rng, B, n, sizes):
    """Small-integer costs with integer u: ties in every column and every row."""
    cost = rng.integers(0, 6, size=(B, n, n)).astype(np.float32)
    u_target = rng.integers(-2, 3, size=(B, n)).astype(np.float32)
    u_pred = (u_target + rng.integers(-1, 2, size=(B, n))).astype(np.float32)
    return pad(cost, u_pred, u_target, sizes)


def sparse_inf_case(rng, B, n, sizes):
    """uniform_case on the grid with about 10 % of the entries +inf.  Every valid row and every valid column
    keeps a finite entry, so v stays finite and no inf - inf arises; the padding stays finite."""
    assert n >= 257
    cost, u_pred, u_target = uniform_case(rng, B, n, sizes)
    cost[rng.random(size=(B, n, n)) < 0.1] = np.inf
    pad(cost, u_pred, u_target, sizes)
    for b, nb in enumerate(sizes):
        finite = np.isfinite(cost[b, :nb, :nb])
        assert finite.any(axis=0).all() and finite.any(axis=1).all(), (b, "a row or column of +inf")
        assert not finite.all()
    return cost, u_pred, u_target


def pad(cost, u_pred, u_target, sizes):
    for b, nb in enumerate(sizes):
        cost[b, nb:, :] = -7.0
        cost[b, :, nb:] = -7.0
        u_pred[b, nb:] = 3.0
        u_target[b, nb:] = -3.0
    return cost, u_pred, u_target


RECIPES = dict(uniform=uniform_case, integer=integer_case, inf=sparse_inf_case)

# label -> (recipe, seed, B, n, sizes): the cases above n = 257, regenerated where they are needed
LARGE_SPECS = {
    "uniform-n1025-B8": ("uniform", 2024110101, 8, 1025, [1025] * 8),
    "uniform-n1028-mixed": ("uniform", 2024110102, 8, 1028, [1028, 1025, 1, 513, 1024, 64, 1027, 1000]),
    "uniform-n4097-B1": ("uniform", 2024110103, 1, 4097, [4097]),
    "uniform-n4100-mixed": ("uniform", 2024110104, 3, 4100, [4100, 4097, 2049]),
    "integer-n1025-B2": ("integer", 2024110105, 2, 1025, [1025, 1024]),
    "inf-n1028-B2": ("inf", 2024110106, 2, 1028, [1028, 1025]),
    "uniform-n1028-B2": ("uniform", 2024110107, 2, 1028, [1028, 1025]),
}
LARGE_REF_LABELS = ("uniform-n1028-B2", "inf-n1028-B2")  # the cases train_loss_large_ref.npz covers


def large_case(label):
    """The inputs of LARGE_SPECS[label], drawn afresh from the case's own seed."""
    kind, seed, B, n, sizes = LARGE_SPECS[label]
    sizes = np.asarray(sizes, dtype=np.int32)
    cost, u_pred, u_target = RECIPES[kind](np.random.default_rng(seed), B, n, sizes)
    return dict(label=label, kind=kind, seed=seed, B=B, n=n, cost=cost, u_pred=u_pred, u_target=u_target,
                sizes=sizes)


def input_crc(m):
    """CRC32 over the bytes of cost, u_pred, u_target and sizes: tells a different NumPy random stream from a
    different result."""
    crc = 0
    for key in ("cost", "u_pred", "u_target", "sizes"):
        crc = zlib.crc32(np.ascontiguousarray(m[key]).tobytes(), crc)
    return crc


def restate_instance(C, u, t, nb, batch, weights=WEIGHTS):
    """One instance: C (n, n), u, t (n,) float32 padded; nb valid; batch = B of the loss mean."""
    f32, f64 = np.float32, np.float64
    C = np.ascontiguousarray(C[:nb, :nb], dtype=f32)
    u = np.ascontiguousarray(u[:nb], dtype=f32)
    t = np.ascontiguousarray(t[:nb], dtype=f32)
    cm = C - u[:, None]
    a = cm.argmin(axis=0)  # first occurrence = lowest row
    v = cm[a, np.arange(nb)]
    h = np.maximum((u[:, None] + v[None, :]) - C, f32(0))
    red = cm - v[None, :]
    order = np.argsort(red.min(axis=1), kind="stable")
    used = np.zeros(nb, dtype=bool)
    assign = np.full(nb, -1, dtype=np.int32)
    for r in order:
        free = np.flatnonzero(~used)
        j = free[np.argmin(red[r][free])]  # first occurrence among the free columns = lowest column
        assign[r] = j
        used[j] = True
    total = 0.0
    for i in range(nb):
        total += float(C[i, assign[i]])
    pos = h > 0
    R = pos.sum(axis=1).astype(np.int64)
    K = pos.sum(axis=0).astype(np.int64)
    cnt = np.bincount(a, minlength=nb).astype(np.int64)
    ksum = np.bincount(a, weights=K, minlength=nb).astype(np.int64)
    d = u - t
    q = d * d
    w = np.asarray(weights, dtype=f32).astype(f64)  # the weights are float32 numbers, in the reference too
    dn = f64(nb)
    gap_g = (cnt - 1).astype(f64)
    feas_g = (R - ksum).astype(f64) / (dn * dn)
    reg_g = 2.0 * (u.astype(f64) - t.astype(f64)) / dn
    g64 = (w[0] * gap_g + w[1] * feas_g + w[2] * reg_g) / f64(batch)
    # what a float32 evaluation of the same gradient may lose: its terms and their absolute sum
    g_terms = 1 + cnt + R + ksum + 1
    g_abs = (w[0] * (1 + cnt) + w[1] * (R + ksum) / (dn * dn) + w[2] * np.abs(reg_g)) / f64(batch)
    return dict(
        v=v, a=a.astype(np.int32), assign=assign, primal_upper=f32(total), order=order,
        dual64=u.astype(f64).sum() + v.astype(f64).sum(), dual_abs=np.abs(u).astype(f64).sum() + np.abs(v).astype(f64).sum(),
        feas64=h.astype(f64).sum() / (dn * dn), ureg64=q.astype(f64).sum() / dn,
        g64=g64, g_terms=g_terms, g_abs=g_abs, cnt=cnt, R=R, K=K, ksum=ksum)


def restate(cost, u, t, sizes, weights=WEIGHTS):
    """A padded batch: per-instance results stacked, padded to n with 0 (v, g64) or -1 (a, assign)."""
    B, n = u.shape
    out = dict(v=np.zeros((B, n), np.float32), a=np.full((B, n), -1, np.int32), assign=np.full((B, n), -1, np.int32),
               g64=np.zeros((B, n)), g_terms=np.zeros((B, n), np.int64), g_abs=np.zeros((B, n)),
               primal_upper=np.zeros(B, np.float32), dual64=np.zeros(B), dual_abs=np.zeros(B), feas64=np.zeros(B),
               ureg64=np.zeros(B))
    for b in range(B):
        nb = int(sizes[b])
        r = restate_instance(cost[b], u[b], t[b], nb, B, weights)
        for key in ("v", "a", "assign", "g64", "g_terms", "g_abs"):
            out[key][b, :nb] = r[key]
        for key in ("primal_upper", "dual64", "dual_abs", "feas64", "ureg64"):
            out[key][b] = r[key]
    return out


def sum_bound(terms, abs_sum):
    """The standard bound of a recursive float32 summation of `terms` numbers (Higham, Accuracy and Stability,
    eq. 4.4, first order), with two more roundings for what is done to the sum afterwards."""
    return (np.asarray(terms, dtype=np.float64) + 2) * F32_EPS * np.asarray(abs_sum, dtype=np.float64)


def reference_bounds(r, sizes):
    """Bounds on |float32 reference - float64 value| for dual_lower, feas, u_reg and grad_u of restate()."""
    nb = np.asarray(sizes, dtype=np.float64)
    return dict(dual=sum_bound(2 * nb, r["dual_abs"]), feas=sum_bound(nb * nb, r["feas64"]),
                # each squared difference carries two roundings of its own
                ureg=sum_bound(nb + 2, r["ureg64"]),
                # the terms of the gradient carry up to four roundings of their own (1/n_b^2, 2 d, / n_b, 0.1)
                grad=sum_bound(r["g_terms"] + 4, r["g_abs"]))


def ulp32(x):
    """The float32 unit in the last place at the magnitude of the float64 value(s) x."""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def within_one_ulp(got32, want64):
    """|got - want| <= 1 float32 ulp at want, elementwise; an exact 0 must be 0."""
    got = np.asarray(got32, dtype=np.float64)
    want = np.asarray(want64, dtype=np.float64)
    ok = np.abs(got - want) <= ulp32(want)
    return np.where(want == 0.0, got == 0.0, ok)


def bits_equal32(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


class TrainLossCases:
    def __init__(self, path=GOLDEN):
        self.z = np.load(path, allow_pickle=False)
        self.meta = json.loads(str(self.z["meta"]))
        self._restated = {}

    def __len__(self):
        return len(self.meta)

    def labels(self):
        return [m["label"] for m in self.meta]

    def case(self, k):
        m = dict(self.meta[k])
        for key in self.z.files:
            if key.startswith(f"c{k}_"):
                m[key[len(f"c{k}_"):]] = self.z[key]
        if "cost_q" in m:
            m["cost"] = cost_from_grid(m.pop("cost_q"))
        return m

    def restated(self, k):
        """restate() of case k, computed once and shared."""
        if k not in self._restated:
            m = self.case(k)
            self._restated[k] = restate(m["cost"], m["u_pred"], m["u_target"], m["sizes"])
        return self._restated[k]
