"""Everything taken from the reference, in one place -- TEST INFRASTRUCTURE.

This is the only module that knows where the reference lies (REF_ROOT).  It gives

  * load_module(): the reference's Python files, imported by path where they lie (never copied), for the
    fixture generators under tests/golden/ and tools/bench_dual_gnn.py;
  * ctypes front-ends of the two libraries that `make -C oracle ref` compiles from the reference's own C++,
    unmodified, where the reference exists: _ref/liblap_ref.so (LAP/_lapjv_cpp/lapjv.cpp and lapjv_seeded.cpp:
    seeded_raw, dense_raw) and _ref/liblapmod_ref.so (lapmod.cpp behind oracle/lapmod_glue.cpp: lapmod_lib).

liblap_ref.so validates the restatement in jv_oracle.c (tests/golden/make_golden.py,
tests/test_oracle_golden.py) and bench.py times it beside the port on a few instances
(cpu_baseline.port_over_reference).  oracle/_ref/ is git-ignored and travels to the GPU box as prebuilt binaries
only -- no reference source does.
"""
from __future__ import annotations

import ctypes as ct
import importlib.util
import subprocess
import sys
import types
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "_ref" / "liblap_ref.so"
LAPMOD_LIB_PATH = _HERE / "_ref" / "liblapmod_ref.so"
REF_ROOT = Path("/root/reference")

_lib = None
_lapmod_lib = None


def load_module(rel_path, name, package=None, stubs=(), root=None):
    """The reference's Python file `rel_path` (relative to the reference root) as module `name`.

    `package` names a stand-in parent package whose __path__ is the file's directory, so that the file's
    relative imports resolve; the module is then `package.name`.  Every name in `stubs` that is not imported
    yet is answered by an empty module (an import the file makes but the caller never reaches).  `root` is
    another checkout of the reference than REF_ROOT."""
    path = Path(root or REF_ROOT) / rel_path
    for stub in stubs:
        sys.modules.setdefault(stub, types.ModuleType(stub))
    if package is not None:
        if package not in sys.modules:
            pkg = types.ModuleType(package)
            pkg.__path__ = [str(path.parent)]
            sys.modules[package] = pkg
        name = f"{package}.{name}"
    spec = importlib.util.spec_from_file_location(name, str(path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _built(path) -> bool:
    if not path.exists() and REF_ROOT.exists():
        subprocess.run(["make", "-C", str(_HERE), "ref"], check=False, capture_output=True)
    return path.exists()


def available() -> bool:
    return _built(LIB_PATH)


def _load():
    global _lib
    if _lib is None:
        if not available():
            raise FileNotFoundError(f"{LIB_PATH} not built (needs {REF_ROOT})")
        lib = ct.CDLL(str(LIB_PATH))
        dp = ct.POINTER(ct.c_double)
        llp = ct.POINTER(ct.c_longlong)
        lib.lapjv_seeded.restype = ct.c_int
        lib.lapjv_seeded.argtypes = [dp, ct.c_int, ct.c_int, llp, llp, dp, dp, ct.c_double]
        # int lapjv_internal(const uint_t n, cost_t *cost[], int_t *x, int_t *y)  (C++ linkage)
        fn = getattr(lib, "_Z14lapjv_internaljPPdPiS1_")
        fn.restype = ct.c_int
        fn.argtypes = [ct.c_uint, ct.POINTER(dp), ct.POINTER(ct.c_int), ct.POINTER(ct.c_int)]
        lib.lapjv_internal = fn
        _lib = lib
    return _lib


def seeded_raw(C, u, v, eps: float = 1e-12):
    lib = _load()
    C = np.ascontiguousarray(C, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    v = np.ascontiguousarray(v, dtype=np.float64)
    n, m = C.shape
    x = np.full(n, -1, dtype=np.int64)
    y = np.full(m, -1, dtype=np.int64)
    dp = ct.POINTER(ct.c_double)
    llp = ct.POINTER(ct.c_longlong)
    ret = lib.lapjv_seeded(C.ctypes.data_as(dp), n, m, x.ctypes.data_as(llp), y.ctypes.data_as(llp),
                           u.ctypes.data_as(dp), v.ctypes.data_as(dp), float(eps))
    return ret, x, y


def dense_raw(C):
    lib = _load()
    C = np.ascontiguousarray(C, dtype=np.float64)
    n = C.shape[0]
    dp = ct.POINTER(ct.c_double)
    rows = (dp * n)()
    base = C.ctypes.data
    for i in range(n):
        rows[i] = ct.cast(base + i * n * 8, dp)
    x = np.empty(n, dtype=np.int32)
    y = np.empty(n, dtype=np.int32)
    ret = lib.lapjv_internal(n, rows, x.ctypes.data_as(ct.POINTER(ct.c_int)),
                             y.ctypes.data_as(ct.POINTER(ct.c_int)))
    return ret, x, y


def lapmod_lib():
    """liblapmod_ref.so with its prototypes (oracle/lapmod_glue.cpp): lapmod_internal(n, cc, ii, kk, x, y, fp) and
    lapmod_v(n, cc, ii, kk, x, y, v, fp), every array passed as an address."""
    global _lapmod_lib
    if _lapmod_lib is None:
        if not _built(LAPMOD_LIB_PATH):
            raise FileNotFoundError(f"{LAPMOD_LIB_PATH} not built (needs {REF_ROOT})")
        lib = ct.CDLL(str(LAPMOD_LIB_PATH))
        lib.lapmod_internal = lib.lapmod_c
        lib.lapmod_internal.restype = ct.c_int
        lib.lapmod_internal.argtypes = [ct.c_uint] + [ct.c_void_p] * 5 + [ct.c_int]
        lib.lapmod_v.restype = ct.c_int
        lib.lapmod_v.argtypes = [ct.c_uint] + [ct.c_void_p] * 6 + [ct.c_int]
        _lapmod_lib = lib
    return _lapmod_lib
