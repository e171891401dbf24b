"""Synthetic cost families made on the device, as ragged packs (csrc/cost_families.hip).

The families are the reference's dataset families (data/generators.py, SYNTHETIC_FAMILIES) with its default
parameters, restated over a counter-based generator: every value is a pure function of (seed, stream, element) under
Philox4x32-10 (csrc/cost_families.hpp has the rules), so an instance's bits depend on its own (family, n, seed,
parameters) and not on the batch around it or its layout.  The streams are not NumPy's: `solvers.generate_family` and
this module give different matrices of the same families for the same seed."""
from __future__ import annotations

import math
from numbers import Integral, Real

import numpy as np

from lap import _hip

from .features import MAX_BATCH, MAX_N, RaggedPack, _ragged_meta

FAMILY_IDS = {"uniform": 0, "metric": 1, "low_rank": 2, "clustered": 3, "block": 3, "noisy_linear": 4, "tie": 5,
              "sparse": 6}
# name -> ((integer parameter, default) or None, (real parameter, default) or None): params[b] = (first, second, 0, 0)
PARAM_NAMES = {
    "uniform": (None, None),
    "metric": (None, None),
    "low_rank": (("rank", 12), ("sigma", 0.1)),
    "clustered": (("blocks", 4), ("noise", 0.1)),
    "block": (("blocks", 4), ("noise", 0.1)),
    "noisy_linear": (("rank", 1), ("noise", 0.1)),
    "tie": (("bins", 5), ("jitter", 1e-6)),
    "sparse": (None, ("sparsity", 0.3)),
}
DEFAULT_PARAMS = {name: {p[0]: p[1] for p in pair if p is not None} for name, pair in PARAM_NAMES.items()}
MAX_RANK = 64


def _instance_params(b, family, given):
    """(first, second) of instance b as floats, from the family's defaults and the instance's dict."""
    given = {} if given is None else dict(given)
    out = []
    for slot, spec in enumerate(PARAM_NAMES[family]):
        if spec is None:
            out.append(0.0)
            continue
        name, default = spec
        value = given.pop(name, default)
        if slot == 0:
            if isinstance(value, bool) or not isinstance(value, Integral):
                raise ValueError(f"instance {b}: {name} must be an integer, not {value!r}")
            if name == "rank" and not 1 <= value <= MAX_RANK:
                raise ValueError(f"instance {b}: rank must be in 1..{MAX_RANK}, not {value}")
            if not 0 <= value <= 2**31 - 1:
                raise ValueError(f"instance {b}: {name} must be in 0..2^31-1, not {value}")
        elif isinstance(value, bool) or not isinstance(value, Real) or not math.isfinite(value):
            raise ValueError(f"instance {b}: {name} must be a finite number, not {value!r}")
        out.append(float(value))
    if given:
        raise ValueError(f"instance {b}: {family} has no parameter {sorted(given)[0]!r}")
    return out


def _check_plan(families, sizes, seeds, params):
    """The host half of synthetic_pack: (names, sizes, seeds, (B, 4) parameters), or KeyError / ValueError."""
    families, sizes, seeds = list(families), list(sizes), list(seeds)
    B = len(families)
    if B < 1:
        raise ValueError("at least one instance expected")
    if B > MAX_BATCH:
        raise ValueError(f"at most {MAX_BATCH} instances per call, not {B}")
    if len(sizes) != B or len(seeds) != B:
        raise ValueError(f"{B} families but {len(sizes)} sizes and {len(seeds)} seeds")
    params = [None] * B if params is None else list(params)
    if len(params) != B:
        raise ValueError(f"{B} families but {len(params)} parameter sets")
    table = np.zeros((B, 4), dtype=np.float64)
    for b, (family, n, seed) in enumerate(zip(families, sizes, seeds)):
        if family not in FAMILY_IDS:
            raise KeyError(f"Unknown family '{family}'. Known families: {sorted(FAMILY_IDS)}")
        if isinstance(n, bool) or not isinstance(n, Integral) or n < 1:
            raise ValueError(f"instance {b}: n must be an integer >= 1, not {n!r}")
        if n > MAX_N:
            raise ValueError(f"instance {b}: n exceeds the {MAX_N} limit of this build: {n}")
        if isinstance(seed, bool) or not isinstance(seed, Integral) or not 0 <= seed < 2**64:
            raise ValueError(f"instance {b}: the seed must be an integer in 0..2^64-1, not {seed!r}")
        table[b, :2] = _instance_params(b, family, params[b])
    return families, [int(n) for n in sizes], [int(s) for s in seeds], table


def synthetic_pack(families, sizes, seeds, device="cuda:0", params=None, padded=False) -> RaggedPack:
    """B synthetic cost matrices made on the device: instance b is the n_b x n_b matrix of family families[b] (a name
    of FAMILY_IDS) from the 64-bit seed seeds[b], with the parameters params[b] (None, or a dict over the names of
    DEFAULT_PARAMS[family]) over the family's defaults.  Returns the RaggedPack that ragged_pack gives for those
    matrices: packed back to back, or with `padded` one (B, N, N) tensor, N the largest size, 0 outside the
    prefixes.  Validates on the host (KeyError for an unknown family, ValueError otherwise) before any device work;
    then one small upload of the plan (3 words per instance, 5 more for the parameters), one call, and no host
    copy of any matrix.  Raises RuntimeError naming the first instance the device refuses."""
    import torch

    from ._call import hip_call
    names, host_sizes, seeds, table = _check_plan(families, sizes, seeds, params)
    lib = _hip.require_device()
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    B, N = len(names), max(host_sizes)
    if padded:
        ld = N
        offsets = np.arange(B, dtype=np.int64) * (N * N)
        C = torch.zeros((B, N, N), dtype=torch.float64, device=device)
    else:
        ld = 0
        sq = np.asarray(host_sizes, dtype=np.int64) ** 2
        offsets = np.concatenate(([0], np.cumsum(sq)[:-1])).astype(np.int64)
        C = torch.empty((int(sq.sum()),), dtype=torch.float64, device=device)
    offs_d, sizes_d, pos_off_d, posenc = _ragged_meta(tuple(host_sizes), ld, offsets, device)
    plan = np.zeros(5 * B + (B + 1) // 2, dtype=np.int64)  # seeds, parameters, families: one copy
    plan[:B] = np.asarray(seeds, dtype=np.uint64).view(np.int64)
    plan[B:5 * B] = table.reshape(-1).view(np.int64)
    plan[5 * B:].view(np.int32)[:B] = [FAMILY_IDS[f] for f in names]
    plan_d = torch.from_numpy(plan).to(device)
    seeds_d, params_d, family_d = plan_d[:B], plan_d[B:5 * B].view(torch.float64), plan_d[5 * B:].view(torch.int32)
    ret = torch.empty((B,), dtype=torch.int32, device=device)
    ws_bytes = int(lib.lapwarm_cost_families_workspace_bytes(B, N))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
    hip_call("lapwarm_generate_costs_ragged", "synthetic_pack", device, C, offs_d, sizes_d, ld, B, N, family_d, seeds_d,
             params_d, ret, ws, ws_bytes)
    bad = torch.nonzero(ret).reshape(-1).tolist()
    if bad:
        raise RuntimeError(f"synthetic_pack: instance {bad[0]} ({names[bad[0]]}, n = {host_sizes[bad[0]]}) was "
                           f"refused with code {int(ret[bad[0]])}")
    return RaggedPack(C, offs_d, sizes_d, pos_off_d, posenc, ld, N, host_sizes)


class SyntheticStream:
    """An endless iterator of batch plans (families, sizes, seeds): `batch` instances each, the family drawn from
    `families`, the size from `sizes` and a 64-bit seed, all from one np.random.default_rng(seed); two streams of one
    seed yield the same plans.  .packs(device) yields the plans as packs made on the device."""

    def __init__(self, families, sizes, batch, seed):
        self.families, self.sizes, self.batch = list(families), [int(n) for n in sizes], int(batch)
        if not self.families or not self.sizes or self.batch < 1:
            raise ValueError("at least one family, one size and one instance per batch expected")
        _check_plan(self.families, [self.sizes[0]] * len(self.families), [0] * len(self.families), None)
        _check_plan([self.families[0]] * len(self.sizes), self.sizes, [0] * len(self.sizes), None)
        self.rng = np.random.default_rng(seed)

    def __iter__(self):
        return self

    def __next__(self):
        f = self.rng.integers(0, len(self.families), size=self.batch)
        s = self.rng.integers(0, len(self.sizes), size=self.batch)
        seeds = self.rng.integers(0, 2**64, size=self.batch, dtype=np.uint64)
        return ([self.families[k] for k in f], [self.sizes[k] for k in s], [int(x) for x in seeds])

    def packs(self, device="cuda:0", padded=False):
        for families, sizes, seeds in self:
            yield synthetic_pack(families, sizes, seeds, device, padded=padded)
