"""Reader of tests/golden/dual_loss_cases.npz and a NumPy restatement of the DualGNN training loss (shared by
tests/golden/make_dual_loss.py, test_dual_loss_fixtures.py and test_gpu_dual_loss.py).  The input recipes, the
greedy and the integer counts are those of train_loss_common.py: v_hint takes the place of u_target in the recipes.

The restatement is written from the definition of the loss, not from the reference's code.  Per instance with n_b
valid rows and columns, B instances in the batch, all terms float32 and every sum in float64:

    v_j, a_j, h_ij, the greedy, cnt_i, R_i, K_j   as in train_loss_common.py
    d_j    = vh_j - v_j                                      (float32)
    v_reg  = sum_j d_j^2 / n_b                               (the squares float32)
    S_i    = sum_{j: a_j = i} d_j                            (float64, in ascending j)
    g_i    = (1/B) [ w0 (cnt_i - 1) + w1 (R_i - sum_{a_j = i} K_j) / n_b^2 + w2 2 S_i / n_b ]
    gvh_j  = (1/B) w2 2 d_j / n_b
"""
import json
from pathlib import Path

import numpy as np

import train_loss_common as tl

GOLDEN = Path(__file__).resolve().parent / "golden" / "dual_loss_cases.npz"
WEIGHTS = tl.WEIGHTS
PER_INSTANCE = ("primal_upper", "dual64", "dual_abs", "feas64", "vreg64")
PER_ELEMENT = ("v", "a", "assign", "g64", "g_terms", "g_abs", "gvh64", "d", "S", "seg_abs", "cnt")


def restate_instance(C, u, vh, nb, batch, weights=WEIGHTS):
    """One instance: C (n, n), u, vh (n,) float32 padded; nb valid; batch = B of the loss mean."""
    f32, f64 = np.float32, np.float64
    # with u as its own target the third term of the OneGNN restatement and its gradient are exactly 0
    r = tl.restate_instance(C, u, u, nb, batch, weights)
    vh = np.ascontiguousarray(vh[:nb], dtype=f32)
    d = vh - r["v"]
    q = d * d
    S = np.zeros(nb, dtype=f64)
    seg_abs = np.zeros(nb, dtype=f64)
    for j in range(nb):  # ascending j
        S[r["a"][j]] += f64(d[j])
        seg_abs[r["a"][j]] += abs(f64(d[j]))
    w = np.asarray(weights, dtype=f32).astype(f64)
    dn = f64(nb)
    r["g64"] = r["g64"] + w[2] * (2.0 * S / dn) / f64(batch)
    r["g_terms"] = r["g_terms"] + r["cnt"]
    r["g_abs"] = r["g_abs"] + w[2] * (2.0 * seg_abs / dn) / f64(batch)
    r.update(d=d, S=S, seg_abs=seg_abs, vreg64=q.astype(f64).sum() / dn,
             gvh64=w[2] * (2.0 * d.astype(f64) / dn) / f64(batch))
    return r


def restate(cost, u, vh, sizes, weights=WEIGHTS):
    """A padded batch: per-instance results stacked, padded to n with 0 or, for a and assign, -1.  An instance of
    size 0 (ret 2 on the device) keeps the padding everywhere and NaN terms."""
    B, n = u.shape
    out = {key: np.zeros((B, n)) for key in PER_ELEMENT}
    out.update(v=np.zeros((B, n), np.float32), d=np.zeros((B, n), np.float32), a=np.full((B, n), -1, np.int32),
               assign=np.full((B, n), -1, np.int32), g_terms=np.zeros((B, n), np.int64), cnt=np.zeros((B, n), np.int64))
    out.update({key: np.zeros(B) for key in PER_INSTANCE})
    out["primal_upper"] = np.zeros(B, np.float32)
    for b in range(B):
        nb = int(sizes[b])
        if nb == 0:
            for key in PER_INSTANCE:
                out[key][b] = np.nan
            continue
        r = restate_instance(cost[b], u[b], vh[b], nb, B, weights)
        for key in PER_ELEMENT:
            out[key][b, :nb] = r[key]
        for key in PER_INSTANCE:
            out[key][b] = r[key]
    return out


def reference_bounds(r, sizes):
    """Bounds on |float32 reference - float64 value| for dual_lower, feas, v_reg, grad_u and grad_v_hint of
    restate(): tl.sum_bound over the terms the reference adds in float32."""
    nb = np.asarray(sizes, dtype=np.float64)
    return dict(dual=tl.sum_bound(2 * nb, r["dual_abs"]), feas=tl.sum_bound(nb * nb, r["feas64"]),
                # each squared difference carries two roundings of its own
                vreg=tl.sum_bound(nb + 2, r["vreg64"]),
                # the terms of grad_u carry up to four roundings of their own (1/n_b^2, 2 d, / n_b, 0.1)
                grad=tl.sum_bound(r["g_terms"] + 4, r["g_abs"]),
                # grad_v_hint is one product: / n_b, 1 / B, 0.1 and the product itself round
                gvh=4 * tl.F32_EPS * np.abs(r["gvh64"]))


def grad_u_allowance(r, sizes, weights=WEIGHTS):
    """What grad_u of the kernel may differ from g64 by beyond its one float32 ulp: S_i can cancel, so the fp64
    summation bound of its run, (cnt_i + 2) 2^-53 sum_{a_j = i} |d_j|, scaled like S_i in the gradient."""
    B = len(sizes)
    dn = np.maximum(np.asarray(sizes, dtype=np.float64), 1.0)[:, None]
    w2 = float(np.float32(weights[2]))
    return (r["cnt"] + 2) * 2.0 ** -53 * r["seg_abs"] * 2.0 * w2 / (dn * B)


def within_one_ulp_plus(got32, want64, extra):
    """tl.within_one_ulp with `extra` added to the allowance; an exact 0 with no allowance must be 0."""
    got = np.asarray(got32, dtype=np.float64)
    want = np.asarray(want64, dtype=np.float64)
    ok = np.abs(got - want) <= tl.ulp32(want) + extra
    return np.where((want == 0.0) & (extra == 0.0), got == 0.0, ok)


def untied(cost, u, v, sizes):
    """No column minimum of C - u and no row minimum of the reduced costs is attained twice, in any instance."""
    for b, nb in enumerate(sizes):
        cm = cost[b, :nb, :nb] - u[b, :nb, None]
        if not ((cm == cm.min(axis=0)).sum(axis=0) == 1).all():
            return False
        red = cm - v[b, None, :nb]
        if not ((red == red.min(axis=1, keepdims=True)).sum(axis=1) == 1).all():
            return False
    return True


class DualLossCases:
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
            m["cost"] = tl.cost_from_grid(m.pop("cost_q"))
        return m

    def restated(self, k):
        """restate() of case k, computed once and shared."""
        if k not in self._restated:
            m = self.case(k)
            self._restated[k] = restate(m["cost"], m["u_pred"], m["v_hint"], m["sizes"])
        return self._restated[k]
