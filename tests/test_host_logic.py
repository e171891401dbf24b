"""CPU tests of the host-side logic: the C ABI library loads and exports every declared symbol
(no compute without a GPU), generators, positional encodings, state-dict compatibility, the
checkpoint loader, error paths that must trigger before any device work, and the rule that the
product never imports the oracle."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd"

# LAP/lap/tests/test_lapjv.py:60-121 (test_square): inputs and the exact expected (opt, x, y)
KNOWN_SQUARE = [
    (np.array([[1000, 2, 11, 10, 8, 7, 6, 5], [6, 1000, 1, 8, 8, 4, 6, 7], [5, 12, 1000, 11, 8, 12, 3, 11],
               [11, 9, 10, 1000, 1, 9, 8, 10], [11, 11, 9, 4, 1000, 2, 10, 9], [12, 8, 5, 2, 11, 1000, 11, 9],
               [10, 11, 12, 10, 9, 12, 1000, 3], [10, 10, 10, 10, 6, 3, 1, 1000]]),
     (17.0, [1, 2, 0, 4, 5, 3, 7, 6], [2, 0, 1, 5, 3, 4, 7, 6])),
    (np.array([[1000, 4, 1], [1, 1000, 3], [5, 1, 1000]]), (3., [2, 0, 1], [1, 2, 0])),
    (np.array([[5, 1000, 3], [1000, 2, 2], [1, 5, 1000]]), (6., [2, 1, 0], [2, 1, 0])),
    (np.array([[1000, 1001, 1000], [1000, 1000, 1001], [1, 2, 3]]), (2001., [2, 1, 0], [2, 1, 0])),
    (np.array([[10, 10, 13], [4, 8, 8], [8, 5, 8]]), (22., [2, 0, 1], [1, 2, 0])),
    (np.array([[11, 10, 6], [10, 11, 11], [11, 12, 15]]), (28., [2, 0, 1], [1, 2, 0])),
    (np.array([[12, 4, 9], [16, 15, 14], [19, 13, 17]]), (37., [1, 0, 2], [1, 0, 2])),
    (np.array([[2, 5, 7], [7, 10, 12], [1, 5, 9]]), (18., [2, 1, 0], [2, 1, 0])),
    (np.array([[10, 6, 14, 1], [17, 18, 17, 15], [14, 17, 15, 8], [11, 13, 11, 4]]),
     (41., [1, 2, 0, 3], [2, 0, 1, 3])),
]
# LAP/lap/tests/test_lapjv.py:132-148 (test_sparse_square): inf entries
KNOWN_INF = (np.array([[11., 20., np.inf, np.inf, np.inf], [12., np.inf, 12., np.inf, np.inf],
                       [np.inf, 11., 10., 15., 9.], [15., np.inf, np.inf, 22., np.inf],
                       [13., np.inf, np.inf, np.inf, 15.]]),
             (71., [0, 2, 1, 3, 4], [0, 2, 1, 3, 4]))


def test_oracle_reproduces_reference_known_answers():
    from oracle import jv
    for cost, (opt, ex, ey) in KNOWN_SQUARE + [KNOWN_INF]:
        got = jv.lapjv(cost)
        assert got[0] == opt and list(got[1]) == ex and list(got[2]) == ey


def test_abi_library_loads_and_exports_every_declared_symbol():
    from lap import _hip
    lib = _hip.load()
    header = (ROOT / "include" / "lapwarm_hip.h").read_text()
    declared = set(re.findall(r"\b(lapjv_seeded|lapwarm_\w+)\s*\(", header))
    assert {"lapjv_seeded", "lapwarm_seeded_batched", "lapwarm_row_features_batched"} <= declared
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in lapwarm_hip.h but not exported"
    assert declared == set(_hip.SIGNATURES), declared ^ set(_hip.SIGNATURES)
    assert lib.lapwarm_seeded_workspace_bytes(32, 2048) > 32 * 2048 * 2048 // 8
    assert lib.lapwarm_seeded_workspace_bytes(1, 0) == 0
    # cold solves: + the candidate lists of the row reduction from n = 512 (128 x 12 + 8 bytes per row) and the
    # hand-over block of their two launches (solver state in global memory: 44 bytes per row)
    assert lib.lapwarm_lapjv_workspace_bytes(3, 256) == lib.lapwarm_seeded_workspace_bytes(3, 256)
    extra = lib.lapwarm_lapjv_workspace_bytes(3, 2048) - lib.lapwarm_seeded_workspace_bytes(3, 2048)
    assert 3 * 2048 * 1544 <= extra <= 3 * 2048 * (1544 + 44) + 16 * 256
    assert lib.lapwarm_lapjv_workspace_bytes(1, 0) == 0
    assert b"gfx950" in lib.lapwarm_build_info()


def test_product_never_imports_the_oracle():
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|libjv_oracle|jv_oracle\.h|oracle/|oracle\.(jv|ref|features_np|one_gnn_ref)",
                     re.MULTILINE)
    n_files = 0
    for path in PKG.rglob("*"):
        if path.suffix in {".py", ".hip", ".hpp", ".cpp", ".h"} or path.name == "Makefile":
            n_files += 1
            assert not pat.search(path.read_text()), path
    assert n_files > 15


def test_no_gpu_means_loud_failure():
    import lap
    from lap import _hip
    if _hip.load().lapwarm_device_count() > 0:
        pytest.skip("GPU present")
    C = np.zeros((4, 4))
    with pytest.raises(RuntimeError, match="no HIP device"):
        lap.lapjv_seeded(C, np.zeros(4), np.zeros(4))
    with pytest.raises(RuntimeError, match="no HIP device"):
        lap.lapjv(C)
    from gnn import compute_row_features
    with pytest.raises(RuntimeError, match="no HIP device"):
        compute_row_features(C)


def test_harness_import_line_resolves_and_out_of_scope_names_raise_on_use():
    # scripts/gnn_benchmark.py:51, verbatim
    from gnn import DualGNN, OneGNN, compute_features, compute_row_features, compute_row_features_torch  # noqa: F401
    with pytest.raises(NotImplementedError, match="DualGNN"):
        DualGNN(hidden_dim=64)
    with pytest.raises(NotImplementedError, match="compute_features"):
        compute_features(np.zeros((2, 2)))
    # scripts/gnn_benchmark.py:47
    from solvers import SciPySolver, SeededLAPSolver, LAPSolver, time_solver_rigorous  # noqa: F401
    from solvers.advanced_dual import project_feasible, reduce_costs, check_dual_feasible  # noqa: F401
    assert (LAPSolver().name, SeededLAPSolver().name) == ("LAP", "SeededLAP")
    from solvers import WarmStartLAPSolver
    w = WarmStartLAPSolver()
    assert w.name == "WarmStartLAP" and w.use_lap
    rows, cols, cost = w.solve(np.zeros((0, 0)), np.zeros(0), np.zeros(0))
    assert rows.size == 0 and cost == 0.0


def test_one_hip_runtime_per_process_library_first_then_torch():
    """liblapwarm_hip loaded BEFORE torch must not leave two libamdhip64 copies in the process
    (torch then reports no GPU).  Fresh interpreter: load the library, import torch, count."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from lap import _hip\n"
            "_hip.load(); a = _hip.hip_runtimes_in_process()\n"
            "import torch; b = _hip.hip_runtimes_in_process()\n"
            "print(len(a), len(b), a == b)\n" % str(PKG))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["1", "1", "True"], r.stdout


def test_launcher_beats_the_harness_sys_path_insert(tmp_path):
    """The reference's scripts insert their repository root at sys.path[0] (scripts/gnn_benchmark.py:21-22),
    which shadows PYTHONPATH.  run_harness.py must still bind `solvers` / `gnn` / `lap` to this package:
    a stand-in harness with decoy packages of the same names next to it."""
    root = tmp_path / "refroot"
    for name in ("gnn", "solvers", "lap"):
        (root / name).mkdir(parents=True)
        (root / name / "__init__.py").write_text("DECOY = True\n")
    (root / "scripts").mkdir()
    (root / "scripts" / "harness.py").write_text(
        "import sys, json\n"
        "from pathlib import Path\n"
        "project_root = Path(__file__).parent.parent\n"
        "sys.path.insert(0, str(project_root))\n"
        "from solvers import SciPySolver, SeededLAPSolver, LAPSolver, time_solver_rigorous\n"
        "from gnn import DualGNN, OneGNN, compute_features, compute_row_features, compute_row_features_torch\n"
        "import lap, gnn, solvers\n"
        "print(json.dumps({'argv': sys.argv[1:], 'files': [m.__file__ for m in (lap, gnn, solvers)],\n"
        "                  'decoy': [hasattr(m, 'DECOY') for m in (lap, gnn, solvers)]}))\n")
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, str(PKG / "run_harness.py"), str(root / "scripts" / "harness.py"), "--sizes", "64"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["argv"] == ["--sizes", "64"] and rec["decoy"] == [False, False, False]
    assert all(f.startswith(str(PKG)) for f in rec["files"])


def test_argument_errors_precede_device_work():
    import lap
    with pytest.raises(ValueError, match="2-dimensional"):
        lap.lapjv(np.zeros(3))
    with pytest.raises(ValueError, match="Square cost array expected"):
        lap.lapjv(np.zeros((3, 2)))
    with pytest.raises(ValueError, match="u/v sizes must match C"):
        lap.lapjv_seeded(np.zeros((3, 3)), np.zeros(2), np.zeros(3))
    with pytest.raises(ValueError):
        lap.lapjv_seeded(np.zeros((3, 3), dtype=np.float32), np.zeros(3), np.zeros(3))
    with pytest.raises(NotImplementedError):
        lap.lapmod()
    assert lap.LARGE == 1000000 and lap.__all__ == ['lapjv', 'lapjv_seeded', 'lapmod', 'FP_1', 'FP_2', 'FP_DYNAMIC', 'LARGE']
    from gnn import compute_row_features, ROW_FEATURE_DIM
    assert compute_row_features(np.zeros((0, 0))).shape == (0, 0) and ROW_FEATURE_DIM == 21


def test_positional_encodings_match_reference(features_cases):
    from gnn import positional_encodings
    z = features_cases
    for key in [str(s) for s in z["labels"]]:
        want = z[f"feat__{key}"][:, 13:]
        assert np.array_equal(positional_encodings(want.shape[0]), want), key


def test_onegnn_state_dict_is_checkpoint_compatible(onegnn_cases):
    from gnn import OneGNN
    z = onegnn_cases
    for tag, H, L, nparams in (("h64l2", 64, 2, 25026), ("h192l4", 192, 4, 359234)):
        ref = {k.split("__", 2)[2]: z[k].shape for k in z.files if k.startswith(f"sd__{tag}__")}
        model = OneGNN(21, hidden=H, layers=L)
        mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        assert mine == ref
        assert sum(p.numel() for p in model.parameters()) == nparams
    with pytest.raises(ValueError):
        OneGNN(21, layers=0)


def test_checkpoint_loader_accepts_both_schemas(tmp_path):
    from gnn import OneGNN, load_checkpoint
    torch.manual_seed(1)
    m = OneGNN(21, hidden=32, layers=3)
    flat = {"model_state_dict": m.state_dict(), "architecture": "one_gnn", "hidden_dim": 32, "layers": 3,
            "dropout": 0.1, "row_feat_dim": 21, "features": "full"}
    nested = {"epoch": 3, "model_state_dict": m.state_dict(), "best_metric": 0.5,
              "config": {"architecture": "one_gnn", "hidden_dim": 32, "layers": 3, "dropout": 0.1,
                         "topk": 8, "row_feat_dim": 21, "heads": 4}}
    for name, ck in (("flat.pt", flat), ("nested.pt", nested)):
        torch.save(ck, tmp_path / name)
        model, info = load_checkpoint(tmp_path / name, "cpu")
        assert info["hidden_dim"] == 32 and info["layers"] == 3 and model.topk == 16  # topk never restored
        for k, v in m.state_dict().items():
            assert torch.equal(model.state_dict()[k], v)
    torch.save({"model_state_dict": m.state_dict(), "architecture": "dual_gnn"}, tmp_path / "d.pt")
    with pytest.raises(ValueError):
        load_checkpoint(tmp_path / "d.pt", "cpu")


def test_generators_are_deterministic_and_in_domain():
    from solvers import generators as g
    a, names = g.mixed_batch(8, 32, seed=5)
    b, _ = g.mixed_batch(8, 32, seed=5)
    assert np.array_equal(a, b) and names == ["uniform"] * 2 + ["sparse"] * 2 + ["metric"] * 2 + ["clustered"] * 2
    assert np.array_equal(g.generate_uniform_costs(16, seed=42), np.random.RandomState(42).uniform(0, 1, (16, 16)))
    sp = g.generate_family("sparse", 64, 3)
    assert sp.max() == 1e6 and (sp < 1e6).any(axis=1).all() and (sp < 1e6).any(axis=0).all()
    m = g.generate_metric_costs(16, 1)
    assert np.allclose(m, m.T) and np.all(np.diag(m) == 0)
    for fam in g.FAMILIES:
        C = g.generate_family(fam, 24, 11)
        assert C.shape == (24, 24) and C.dtype == np.float64 and np.isfinite(C).all()


def test_shard_bounds_cover_the_batch():
    from gnn.sharding import shard_bounds
    for total in (1, 7, 32, 256):
        for world in (1, 2, 3, 8):
            cuts = [shard_bounds(total, world, r) for r in range(world)]
            assert cuts[0][0] == 0 and cuts[-1][1] == total
            assert all(cuts[i][1] == cuts[i + 1][0] for i in range(world - 1))
            sizes = [hi - lo for lo, hi in cuts]
            assert max(sizes) - min(sizes) <= 1


def test_solver_lds_plan_fits_the_cu_for_every_size():
    """Whatever LDS level the launcher picks for a size, the byte count it will request must fit the
    160 KiB of a CU (a mis-sized level fails at launch with 'invalid argument' on the GPU only).
    Internal C++ symbols of the library, by their mangled names."""
    import ctypes as ct
    from lap import _hip
    lib = _hip.load()
    level = lib._ZN7lapwarm16solver_lds_levelEii
    level.restype, level.argtypes = ct.c_int, [ct.c_int, ct.c_int]
    nbytes = lib._ZN7lapwarm16solver_lds_bytesEiii
    nbytes.restype, nbytes.argtypes = ct.c_size_t, [ct.c_int, ct.c_int, ct.c_int]
    seen = set()
    for n in list(range(1, 600)) + list(range(600, 16385, 37)) + [2048, 3634, 3635, 4096, 4427, 4428, 8192, 16384]:
        for ch in (1, 2, 4, 8, 16):
            lv = level(n, ch)
            seen.add(lv)
            assert nbytes(n, ch, lv) <= 160 * 1024, (n, ch, lv, nbytes(n, ch, lv))
    assert {0, 1, 2} <= seen
    assert nbytes(8192, 16, 8) <= 160 * 1024  # the 512 x 16 large-row geometry (two row slots)


def test_cooperative_plan_per_size():
    """Host side of the cooperative shortest-path kernel (no GPU needed): it is planned from the size
    where the solver state leaves one CU's LDS, with at most 32 members of 64 x {4,8} positions
    that cover the row, and the solver workspace grows by its mailbox + hand-over block there."""
    from lap import _hip
    lib = _hip.load()
    assert lib.lapwarm_coop_members(2048) == 0 and lib.lapwarm_coop_members(4096) == 0  # single-workgroup kernel
    assert lib.lapwarm_coop_members(4427) == 0 and lib.lapwarm_coop_members(4428) > 0
    assert lib.lapwarm_coop_members(8192) == 32 and lib.lapwarm_coop_members(16384) == 32
    for n in (4428, 4608, 5000, 8191, 8192, 8193, 9216, 12000, 16384):
        g = lib.lapwarm_coop_members(n)
        per_lane = 4 if n <= 8192 else 8
        assert 1 <= g <= 32 and g * 64 * per_lane >= n > (g - 1) * 64 * per_lane, (n, g)
        assert lib.lapwarm_solver_uses_helpers(n) == 0  # the helper workgroups belong to the other kernel
    assert lib.lapwarm_coop_members(0) == 0 and lib.lapwarm_coop_members(20000) == 0
    # workspace: monotone in the batch and large enough for the global solver state the hand-over uses
    for n in (4428, 8192):
        one, four = lib.lapwarm_seeded_workspace_bytes(1, n), lib.lapwarm_seeded_workspace_bytes(4, n)
        assert four > one >= n * (3 * 8 + 2 * 4 + 2 * 8 + 7 * 4) + n * ((n + 31) // 32) * 4


def test_solver_geometry_and_timing_helper():
    from solvers import time_solver_rigorous
    calls = []
    out = time_solver_rigorous(lambda: calls.append(1), num_warmups=2, num_repeats=4)
    assert out["success"] and out["num_samples"] == 4 and len(calls) == 6

    def boom():
        raise RuntimeError("x")
    assert time_solver_rigorous(boom, 1, 2) == {"success": False, "error": "x"}


# lapwarm_{kind}_workspace_bytes(batch, n) under default settings, recorded before the workspace layouts
# and the solve plan were unified; the byte counts are part of the ABI contract
WS_SIZES_N = (1, 64, 255, 256, 511, 512, 1024, 1025, 2048, 3634, 3635, 4096, 4427, 4428, 8192, 8193, 16384)
WS_SIZES = {
    "seeded": {
        1: [2304, 3328, 17152, 17152, 49920, 49920, 164608, 170240, 590592, 1935360, 1935616, 2409472, 2801408,
             2804992, 9016320, 9052160, 34804736],
        3: [2816, 8960, 50432, 50432, 148736, 148736, 492800, 506880, 1770752, 5803264, 5804544, 7226880, 8397312,
             8406272, 27046400, 27147008, 104411648],
        32: [10240, 90624, 531200, 532992, 1578752, 1581568, 5251584, 5388288, 18883072, 61874176, 61892352,
             77079296, 89541888, 89634560, 288484096, 289523200, 1113713408],
    },
    "lapjv": {
        1: [2304, 3328, 17152, 17152, 49920, 863744, 1791488, 1800960, 3843584, 7546880, 7548672, 8734208, 9637376,
             9641984, 21664768, 21702400, 60101632],
        3: [2816, 8960, 50432, 50432, 148736, 2588928, 5372160, 5393152, 11528448, 22636800, 22642688, 26200320,
             28904192, 28916992, 64991744, 65097216, 180302336],
        32: [10240, 90624, 531200, 532992, 1578752, 27605760, 57293568, 57481984, 122960640, 241428992, 241496576,
             279460608, 308277248, 308413184, 693234432, 694322944, 1923214080],
    },
    "sweep": {
        1: [768, 2048, 20480, 20480, 73728, 73728, 278528, 287744, 1081344, 3372800, 3373568, 4259840, 4994048,
             4995328, 8519680, 8062464, 8650752],
        3: [768, 6144, 61440, 61440, 220928, 221184, 835584, 861696, 3244032, 7675392, 7677440, 8650752, 8288000,
             8289792, 8847360, 8455680, 9437184],
        32: [768, 65536, 652800, 655360, 2354688, 2359296, 8912896, 6297600, 9437184, 9303040, 9305600, 10485760,
             11333120, 11335680, 12582912, 12584448, 16777216],
    },
    "oracle_duals": {
        1: [3584, 6656, 42752, 42752, 133888, 133888, 463616, 478976, 1712896, 5220608, 5221632, 6570752, 7687680,
             7689728, 13140736, 12456448, 13697792],
        3: [3584, 18432, 126720, 126720, 399872, 400128, 1389312, 1430016, 5137152, 11994368, 11997440, 13517568,
             13018368, 13020928, 14353152, 13767168, 16319232],
        32: [5632, 190976, 1341184, 1346048, 4254464, 4262400, 14813696, 10892544, 17041920, 19073792, 19079424,
             21498368, 23235840, 23240704, 30411264, 30415360, 48237056],
    },
}


def test_workspace_sizes_are_unchanged():
    import ctypes as ct
    from lap import _hip
    lib = _hip.load()
    for kind, per_batch in WS_SIZES.items():
        f = getattr(lib, f"lapwarm_{kind}_workspace_bytes")
        f.restype, f.argtypes = ct.c_size_t, [ct.c_int, ct.c_int]
        for batch, want in per_batch.items():
            got = [f(batch, n) for n in WS_SIZES_N]
            assert got == want, (kind, batch, [(n, g, w) for n, g, w in zip(WS_SIZES_N, got, want) if g != w])


# solver_lds_bytes(n, ch, level) for n in WS_SIZES_N, recorded from the library before the records the solver
# kernels share were named.  The kernel's LDS carving and the host's byte count are still two pieces of code
# that have to agree: solver_lds_bytes sits next to the carving in jv_solver.hip.  Levels 0..2 do not depend
# on ch (every ch in LDS_SIZES_CH gave the row below); level 8 exists for the 512 x 16 geometry of n = 8192 only.
LDS_SIZES_CH = (1, 2, 4, 8, 16)
LDS_SIZES = {
    0: [
        1816, 1816, 1936, 1936, 2096, 2096, 2416, 2456, 3056, 4056, 4056, 4336, 4576, 4576, 6896, 6936, 12016],
    1: [
        1860, 4128, 11124, 11160, 20500, 20536, 39288, 39364, 76792, 134888, 134924, 151800, 163956, 163992,
        301816, 301892, 601848],
    2: [
        1868, 4640, 13164, 13208, 24588, 24632, 47480, 47564, 93176, 163960, 164004, 184568, 199372, 199416,
        367352, 367436, 732920],
}
LDS_SIZE_LARGE_ROWS = ((8192, 16, 8), 137984)


def test_solver_lds_sizes_are_unchanged():
    import ctypes as ct
    from lap import _hip
    lib = _hip.load()
    nbytes = lib._ZN7lapwarm16solver_lds_bytesEiii
    nbytes.restype, nbytes.argtypes = ct.c_size_t, [ct.c_int, ct.c_int, ct.c_int]
    for level, want in LDS_SIZES.items():
        for ch in LDS_SIZES_CH:
            got = [nbytes(n, ch, level) for n in WS_SIZES_N]
            assert got == want, (level, ch, [(n, g, w) for n, g, w in zip(WS_SIZES_N, got, want) if g != w])
    args, want = LDS_SIZE_LARGE_ROWS
    assert nbytes(*args) == want, (args, nbytes(*args), want)


def test_forced_cooperative_geometry_without_an_instantiation_is_not_planned():
    """LAPWARM_COOP_CH=1 at n = 2048 gives 32 members and 3 granule loads per lane: no coop_ssp_kernel<1, 3>
    exists, so the solve takes the one-workgroup path; n = 640 (10 members, <1, 1>) stays cooperative.
    A fresh interpreter: the library reads its settings once."""
    import os
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from lap import _hip\n"
            "lib = _hip.load()\n"
            "print(lib.lapwarm_coop_members(2048), lib.lapwarm_coop_members(640))\n" % str(PKG))
    env = dict(os.environ, LAPWARM_COOP_MIN_N="1", LAPWARM_COOP_CH="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["0", "10"], r.stdout


def test_cooperative_configurations_are_what_the_planner_plans():
    """tests/coop_configs_common.py: every row's (environment, n) gives the member count and the
    coop_ssp_kernel<CH, NL> it names, the rows together reach all twelve instantiations of kCoopKernels, and
    the switch sweeps reach the plan (agent-scope stores, relaunch pairs, helpers per instance) at every size.
    One fresh interpreter per distinct environment: the library reads its settings once."""
    import coop_configs_common as cc
    assert {c.kernel for c in cc.CONFIGS} == {(1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2), (4, 3), (8, 1), (8, 2),
                                              (8, 3), (16, 1), (16, 2)} == cc.COOP_KERNELS
    # kCoopKernels itself: {ch, nl, launch_cfg<ch, nl>} entries in csrc/coop_ssp.hip
    src = (PKG / "csrc" / "coop_ssp.hip").read_text()
    table = src[src.index("kCoopKernels[] = {"):]
    shipped = re.findall(r"\{(\d+), (\d+), launch_cfg<(\d+), (\d+)>\}", table[:table.index("};")])
    assert len(shipped) == 12 and all(e[:2] == e[2:] for e in shipped), shipped
    assert {(int(ch), int(nl)) for ch, nl, _, _ in shipped} == cc.COOP_KERNELS
    assert len({c.label for c in cc.CONFIGS}) == len(cc.CONFIGS)
    envs = []
    for c in cc.CONFIGS:
        if c.env not in envs:
            envs.append(c.env)
    assert len(envs) == 6  # default, MIN_N alone, MIN_N + CH in {1, 2, 8, 16}
    for env in envs:
        rows = [c for c in cc.CONFIGS if c.env == env]
        for c, (members, plan) in zip(rows, cc.planned(env, [c.n for c in rows])):
            ch, nl = c.kernel
            assert members == c.members > 0, (c.label, members)
            assert (4 * members + 87) // 64 == nl, (c.label, members)
            assert (members - 1) * 64 * ch < c.n <= members * 64 * ch, c.label  # with n, the member count pins CH
            assert (plan["coop_ch"], plan["coop_nl"], plan["coop_members"]) == (ch, nl, members), (c.label, plan)
            assert plan["shape"] == 2 and plan["helper"] == 0, (c.label, plan)  # the cooperative chain
            assert plan["coop_pairs"] == 96 and plan["coop_xcd_stores"] == 1, (c.label, plan)
    for s in cc.SWITCH_SWEEPS:
        assert len(s.sizes) == len(s.members)
        for n, want, (members, plan) in zip(s.sizes, s.members, cc.planned(s.env, s.sizes)):
            assert members == want == plan["coop_members"], (s.label, n, members)
            assert (plan["shape"] == 2) == (want > 0), (s.label, n, plan)
            for field, value in s.plan.items():
                assert plan[field] == value, (s.label, n, field, plan)


# ---- the solve plan (csrc/solve_plan.hip) against tests/golden/solve_plans.json, recorded from the library
# before the planner moved out of the kernel files: a wrong threads / ch / ldsl / tb / helper / cooperative
# decision still solves correctly, so only a table catches it

def _golden_plans(key):
    import json
    return json.loads((ROOT / "tests" / "golden" / "solve_plans.json").read_text())[key]


def _assert_same_plans(got, want, points, where):
    for args, g, w in zip(points, got["index"], want["index"]):
        assert got["plans"][g] == want["plans"][w], (where, "mode, batch, n, hint, lists, cus", args,
                                                     got["plans"][g], want["plans"][w])
    assert len(got["index"]) == len(want["index"]) == len(points)
    assert got["queries"] == want["queries"], where


def test_solve_plan_table_is_unchanged():
    """Every field of lapwarm::plan_solve over mode x WS_SIZES_N x threads_hint x lists x (batch, n_cus), default
    environment; (128, 256) and (129, 256) sit on either side of the helper guard batch * 2 <= n_cus."""
    import solve_plan_common as spc
    from lap import _hip
    assert spc.GRID_N == WS_SIZES_N
    points = list(spc.grid())
    assert len(points) == 2 * len(WS_SIZES_N) * 5 * 2 * 4
    want = _golden_plans("default")
    _assert_same_plans(spc.record(_hip.load(), points), want, points, "default")
    helpers = {p[13] for p in want["plans"]}
    shapes = {p[0] for p in want["plans"]}
    assert helpers == {0, 1} and shapes == {0, 1, 2}  # the table does cover the decisions it is there for


@pytest.mark.parametrize("setting", ["LAPWARM_COOP_MIN_N=1", "LAPWARM_HELPER=0", "LAPWARM_ARR_LISTS=0"])
def test_solve_plan_table_under_a_knob_is_unchanged(setting):
    """The same for n in (64, 640, 2048, 4428, 8192) with one knob off its default, plus what the workspace
    layout asks beside the plan.  A fresh interpreter: the library reads its settings once."""
    import json
    import os
    import subprocess
    import sys
    import solve_plan_common as spc
    name, value = setting.split("=")
    r = subprocess.run([sys.executable, spc.__file__], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **{name: value}))
    assert r.returncode == 0, r.stderr[-2000:]
    want = _golden_plans(setting)
    _assert_same_plans(json.loads(r.stdout), want, list(spc.env_grid()), setting)
