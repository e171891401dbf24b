"""Writes tests/golden/lapmod_cases.npz and lapmod_long_rows.npz: sparse LAPMOD inputs and what the reference's
lapmod_internal returns for them with FP_1, FP_2 and FP_DYNAMIC.  The second file holds the cases of
long_row_cases(), drawn from a generator of their own, and for dec_single193 the two counts of arr_first_values();
every condition those cases are there for is asserted and printed.  A committed file is loaded first and every key
of it must equal what is about to be written: stored cases never move.

    python tests/golden/make_lapmod.py [LDS_MAX_N]          (from the repo root)

calls lapmod_internal of oracle/_ref/liblapmod_ref.so (the reference's LAP/_lapjv_cpp/lapmod.cpp, compiled by
oracle/Makefile where the reference exists; oracle.ref.lapmod_lib) and stores data only.  Per case `c`: n, cc (divided by ccscale where it is stored as integers), ii, kk; solvable (a perfect matching
exists), strict (unsolvable and certain to end with ret = 1 on the device: every row has an entry, and row 0 is
not left holding an empty column by the column reduction), aug (the reference reaches the augmentation phase: an
fp_version outside the enum makes it return -2 exactly then); per fp_version v in 1, 2, 3: ret_v, x_v, y_v, and
for solvable cases and v in 1, 2 the final column duals v_v (the phases called with a caller-owned v)
(unsolvable cases are run with FP_1 only and when it is FP_1 that FP_DYNAMIC selects: find_path_sparse_2 reads
outside its arrays there).  LDS_MAX_N is lapwarm_lapmod_lds_max_n() of the built library (default 3395).
"""
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
INF = np.inf
sys.path.insert(0, str(HERE.parents[1]))
from oracle.ref import lapmod_lib  # noqa: E402


def ref_solve(lib, n, cc, ii, kk, fp):
    cc = np.ascontiguousarray(cc, dtype=np.float64)
    ii = np.ascontiguousarray(ii, dtype=np.uint32)
    kk = np.ascontiguousarray(kk, dtype=np.uint32)
    x = np.full(n, -7, dtype=np.int32)
    y = np.full(n, -7, dtype=np.int32)
    t = time.perf_counter()
    ret = lib.lapmod_internal(n, cc.ctypes.data, ii.ctypes.data, kk.ctypes.data, x.ctypes.data, y.ctypes.data, fp)
    return ret, x, y, time.perf_counter() - t


def ref_duals(lib, n, cc, ii, kk, fp):
    """(ret, x, y, v) of the reference's phases with a caller-owned v."""
    cc = np.ascontiguousarray(cc, dtype=np.float64)
    ii = np.ascontiguousarray(ii, dtype=np.uint32)
    kk = np.ascontiguousarray(kk, dtype=np.uint32)
    x, y, v = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32), np.full(n, np.nan)
    ret = lib.lapmod_v(n, cc.ctypes.data, ii.ctypes.data, kk.ctypes.data, x.ctypes.data, y.ctypes.data,
                       v.ctypes.data, fp)
    return ret, x, y, v


def from_masked(cost):
    cost = np.asarray(cost, dtype=np.float64)
    mask = np.isfinite(cost)
    n = cost.shape[0]
    ii = np.zeros(n + 1, dtype=np.int64)
    ii[1:] = np.cumsum(mask.sum(axis=1))
    kk = np.tile(np.arange(cost.shape[1]), n)[mask.ravel()]
    return n, cost[mask], ii, kk


def random_sparse(rng, n, k, draw, single_rows=0.0):
    """k random columns per row plus a hidden permutation (so a perfect matching exists); `single_rows` of the
    rows keep the permutation entry only."""
    perm = rng.permutation(n)
    cost = np.full((n, n), INF)
    for i in range(n):
        cols = [perm[i]]
        if rng.random() >= single_rows:
            cols = np.union1d(cols, rng.choice(n, size=min(k, n), replace=False))
        cost[i, cols] = draw(len(cols))
    return cost


def has_perfect_matching(n, ii, kk):
    match = [-1] * n

    def aug(i, seen):
        for j in kk[ii[i]:ii[i + 1]]:
            if not seen[j]:
                seen[j] = True
                if match[j] < 0 or aug(match[j], seen):
                    match[j] = i
                    return True
        return False
    sys.setrecursionlimit(100000)
    return all(aug(i, [False] * n) for i in range(n))


def certain_ret1(n, cc, ii, kk):
    """Every row has an entry, and the backward pass of the column reduction does not give row 0 an empty column."""
    if np.any(np.diff(ii) == 0):
        return False
    v = np.full(n, 1e6)
    y = np.zeros(n, dtype=np.int64)
    for i in range(n):
        for k in range(ii[i], ii[i + 1]):
            if cc[k] < v[kk[k]]:
                v[kk[k]], y[kk[k]] = cc[k], i
    empty = np.ones(n, dtype=bool)
    empty[kk] = False
    claim0 = np.flatnonzero(y == 0)
    return not empty[claim0.max()] if claim0.size else True


def arr_first_values(n, cc, ii, kk):
    """The column reduction, the reduction transfer and the two ARR passes, serially and in plain Python, after
    DESIGN.md, "Sparse LAPMOD".  Returns (above, far, free): the ARR rows whose first reduced value exceeds LARGE,
    those of them whose first entry below LARGE lies at position >= 64 of the row (the serial scan ignores every
    entry before it), and the rows still free after the second pass."""
    LARGE = 1e6
    v, x, y = np.full(n, LARGE), np.full(n, -1), np.zeros(n, dtype=np.int64)
    for i in range(n):
        for k in range(ii[i], ii[i + 1]):
            if cc[k] < v[kk[k]]:
                v[kk[k]], y[kk[k]] = cc[k], i
    shared = np.zeros(n, dtype=bool)  # rows that claimed more than one column
    for j in reversed(range(n)):
        if x[y[j]] < 0:
            x[y[j]] = j
        else:
            shared[y[j]] = True
            y[j] = -1
    free = []
    for i in range(n):
        if x[i] < 0:
            free.append(i)
        elif not shared[i] and ii[i + 1] - ii[i] > 1:
            others = [cc[k] - v[kk[k]] for k in range(ii[i], ii[i + 1]) if kk[k] != x[i]]
            v[x[i]] -= min([LARGE] + others)
    above = far = 0
    for _ in range(2):
        todo, free, current, visits = free, [], 0, 0
        while current < len(todo):
            visits += 1
            row = todo[current]
            current += 1
            red = [cc[k] - v[kk[k]] for k in range(ii[row], ii[row + 1])]
            j1, v1, j2, v2 = (kk[ii[row]], red[0], -1, LARGE) if red else (0, LARGE, -1, LARGE)
            if red and red[0] > LARGE:
                above += 1
                below = [p for p in range(1, len(red)) if red[p] < LARGE]
                far += bool(below) and below[0] >= 64
            for p in range(1, len(red)):
                if red[p] < v2:
                    if red[p] >= v1:
                        j2, v2 = kk[ii[row] + p], red[p]
                    else:
                        j2, v2, j1, v1 = j1, v1, kk[ii[row] + p], red[p]
            owner, lowered = y[j1], v[j1] - (v2 - v1)
            lowers = lowered < v[j1]
            if visits < current * n:
                if lowers:
                    v[j1] = lowered
                elif owner >= 0 and j2 >= 0:
                    j1, owner = j2, y[j2]
                if owner >= 0 and lowers:
                    current -= 1
                    todo[current] = owner
                elif owner >= 0:
                    free.append(owner)
            elif owner >= 0:
                free.append(owner)
            x[row], y[j1] = j1, row
    return above, far, len(free)


def stored_cases(lds_max):
    """The 45 cases of lapmod_cases.npz, from their own generator: they keep their draws whatever follows."""
    rng = np.random.default_rng(20240611)
    cases = []  # (label, n, cc, ii, kk, kind)

    def add(label, cost, kind=""):
        cases.append((label,) + from_masked(cost) + (kind,))

    k8 = np.array([[1000, 2, 11, 10, 8, 7, 6, 5], [6, 1000, 1, 8, 8, 4, 6, 7], [5, 12, 1000, 11, 8, 12, 3, 11],
                   [11, 9, 10, 1000, 1, 9, 8, 10], [11, 11, 9, 4, 1000, 2, 10, 9], [12, 8, 5, 2, 11, 1000, 11, 9],
                   [10, 11, 12, 10, 9, 12, 1000, 3], [10, 10, 10, 10, 6, 3, 1, 1000]], dtype=np.float64)
    add("known8_dense", k8)
    add("known8_masked", np.where(k8 == 1000, INF, k8))
    for t, m in enumerate([[[1000, 4, 1], [1, 1000, 3], [5, 1, 1000]], [[5, 1000, 3], [1000, 2, 2], [1, 5, 1000]],
                           [[1000, 1001, 1000], [1000, 1000, 1001], [1, 2, 3]], [[10, 10, 13], [4, 8, 8], [8, 5, 8]],
                           [[11, 10, 6], [10, 11, 11], [11, 12, 15]], [[12, 4, 9], [16, 15, 14], [19, 13, 17]],
                           [[2, 5, 7], [7, 10, 12], [1, 5, 9]],
                           [[10, 6, 14, 1], [17, 18, 17, 15], [14, 17, 15, 8], [11, 13, 11, 4]]]):
        add(f"known_square{t}", np.array(m, dtype=np.float64))
    add("known_sparse_square", [[11, 20, INF, INF, INF], [12, INF, 12, INF, INF], [INF, 11, 10, 15, 9],
                                [15, INF, INF, 22, INF], [13, INF, INF, INF, 15]])
    # test_arr_loop.py:63-78: a 7 x 3 COO problem extended to 10 x 10 with cost limit 1e3
    acc = [2.593883482138951146e-01, 3.080381437461217620e-01, 1.976243020727339317e-01, 2.462740976049606068e-01,
           4.203993396282833528e-01, 4.286184525458427985e-01, 1.706431415909629434e-01, 2.192929371231896185e-01,
           2.117769622802734286e-01, 2.604267578125001315e-01]
    ai, aj = [0, 0, 1, 1, 2, 2, 5, 5, 6, 6], [0, 1, 0, 1, 1, 2, 0, 1, 0, 1]
    ext = np.full((10, 10), INF)
    for c, i, j in zip(acc, ai, aj):
        ext[i, j] = c
        ext[7 + j, 3 + i] = 0.0
    for i in range(7):
        ext[i, 3 + i] = 1e3
    for j in range(3):
        ext[7 + j, j] = 1e3
    add("arr_loop", ext)
    z = 0.0
    add("infs_unsolvable0", [[z, z, z, INF, INF], [INF, INF, INF, z, z], [INF, INF, INF, z, z],
                             [INF, INF, INF, z, z], [z, z, z, INF, INF]], "unsolvable")
    add("infs_unsolvable1", [[19, 22, 16, INF, INF], [INF, INF, INF, 4, 13], [INF, INF, INF, 3, 14],
                             [INF, INF, INF, 10, 12], [11, 14, 13, INF, INF]], "unsolvable")
    uniq = np.full((4, 4), INF)
    uniq[:3, :3] = [[1000, 4, 1], [1, 1000, 3], [5, 1, 1000]]
    uniq[3, 3] = 0
    add("inf_unique", uniq)
    add("inf_col", [[z, INF, z, z, INF], [INF, INF, z, z, z], [INF, INF, INF, z, INF], [INF, INF, INF, z, z],
                    [z, INF, z, INF, INF]], "unsolvable")
    add("inf_row", [[z, z, z, z, INF], [INF, INF, z, z, z], [INF, INF, INF, INF, INF], [INF, INF, INF, z, z],
                    [z, z, z, INF, INF]], "unsolvable")

    def ints(hi):
        return lambda m: rng.integers(1, hi + 1, size=m).astype(np.float64)

    def cont(m):
        return rng.random(m) * 100.0

    for n in (1, 2, 3):
        add(f"n{n}_dense_int", rng.integers(1, 6, size=(n, n)).astype(np.float64))
        add(f"n{n}_dense_cont", rng.random((n, n)) * 10.0)
    for n in (63, 64, 65, 257):
        add(f"n{n}_sparse_tie", random_sparse(rng, n, 4, ints(5)), "tie")
        add(f"n{n}_dense_tie", random_sparse(rng, n, (2 * n) // 5, ints(5)), "tie")
        add(f"n{n}_sparse_cont", random_sparse(rng, n, 6, cont))
        add(f"n{n}_dense_cont", random_sparse(rng, n, (2 * n) // 5, cont))
    add("n64_single_rows", random_sparse(rng, 64, 4, ints(5), single_rows=0.25), "tie")
    # an empty column, with row 0 holding the strict minimum of a later column
    ec = random_sparse(rng, 20, 4, ints(5))
    ec[:, 3] = INF
    ec[0, 19] = 0.0
    ec[1, 0] = 1.0  # (the row whose permutation entry was in column 3 keeps an entry)
    for i in range(20):
        if not np.isfinite(ec[i]).any():
            ec[i, (i + 5) % 20 if (i + 5) % 20 != 3 else 4] = 2.0
    add("empty_column", ec, "unsolvable")
    # a column whose only two entries tie
    tc = random_sparse(rng, 32, 4, ints(5))
    tc[:, 7] = INF
    tc[5, 7] = tc[21, 7] = 3.0
    add("tied_column", tc, "tie")
    # the LDS / workspace boundary and a large instance: costs 1..40 keep the row reduction short
    mostly_fine = ints(40)

    add(f"n{lds_max}_lds_bound", random_sparse(rng, lds_max, 4, mostly_fine), "tie")
    add(f"n{lds_max + 1}_above_lds", random_sparse(rng, lds_max + 1, 4, mostly_fine), "tie")
    add("n4096_k16", random_sparse(rng, 4096, 16, mostly_fine), "tie")

    return cases


def long_row_cases():
    """The cases of lapmod_long_rows.npz, from a generator of their own: rows of 64, 65, 128, 129 and 193 entries
    (the device loops take a row in chunks of 64), costs that are inexact in fp64 and reach the path search, and
    unsolvable instances above n = 64."""
    rng = np.random.default_rng(20261021)
    cases = []

    def add(label, cost, kind="long"):
        cases.append((label,) + from_masked(cost) + (kind,))

    def dec(m):  # decimal ties: tenths are no dyadic fractions
        return rng.integers(1, 8, size=m) / 10.0

    add("dec_full129", random_sparse(rng, 129, 129, dec))
    add("dec_full193", random_sparse(rng, 193, 193, dec))
    add("dec_rows64_n130", random_sparse(rng, 130, 63, dec))
    add("dec_rows65_n130", random_sparse(rng, 130, 64, dec))
    add("dec_rows128_n200", random_sparse(rng, 200, 127, dec))
    add("dec_rows129_n200", random_sparse(rng, 200, 128, dec))
    add("dec_sparse130", random_sparse(rng, 130, 4, dec))
    add("lowrank129", np.outer(rng.random(129) * 10.0, rng.random(129) * 10.0) + 0.01 * rng.random((129, 129)))
    # Single-entry rows, built by hand.  A single-entry row that ARR visits lowers its column's v by about 1e6, and
    # the full row it displaces then starts with a reduced value above LARGE where its entry of column 0 costs more
    # than the single one.  Its first entry below LARGE lies behind every lowered column, so position >= 64 needs
    # columns 0..63 lowered: more single-entry rows than `single_rows = 0.2` of 193 gives, in the order of their
    # columns, each at the column's smallest cost (1/10) and below a full row that claims the column first.
    n, first, count = 193, 120, 66
    sr = np.full((n, n), INF)
    for i in range(n):
        if first <= i < first + count:
            sr[i, i - first] = 1 / 10.0
        else:
            sr[i] = dec(n)
    add("dec_single193", sr)
    # an empty column, with row 0 holding the strict minimum of a later column (as `empty_column`)
    ec = random_sparse(rng, 130, 64, dec)
    ec[:, 3] = INF
    ec[0, 129] = 0.0
    assert np.isfinite(ec).any(axis=1).all()  # (the row whose permutation entry was in column 3 keeps its others)
    add("dec_empty_col130", ec, "unsolvable")
    # Hall's condition: two rows hold the same single column, and no column is empty
    hc = random_sparse(rng, 130, 64, dec)
    for i in (41, 97):
        hc[i] = INF
        hc[i, 70] = dec(1)[0]
    assert np.isfinite(hc).any(axis=0).all()
    add("dec_hall130", hc, "unsolvable")
    return cases


def records(lib, cases, times):
    """label__key -> array for every case, and what the assertions of main() need: kind -> [(label, n, aug)], the
    number of solvable cases whose FP_1 and FP_2 assignments differ."""
    out, by_kind, disagree = {}, {}, 0
    for label, n, cc, ii, kk, kind in cases:
        solvable = kind != "unsolvable"
        if n <= 300:  # (the larger ones hold a permutation by construction)
            assert has_perfect_matching(n, ii, kk) == solvable, label
        dyn = 1 if ii[n] / float(n * n) > 0.25 else 2
        aug = ref_solve(lib, n, cc, ii, kk, 99)[0] == -2
        small = n < 32768
        out[f"{label}__n"] = np.int64(n)
        scale = next((q for q in (1, 64) if np.all(cc * q == np.floor(cc * q)) and cc.max() * q < 65536), 0)
        if not scale and np.array_equal(np.rint(cc * 10) / 10.0, cc) and cc.max() * 10 < 65536:
            scale = 10  # tenths: drawn as integers over 10.0, so stored / 10.0 gives their bits back
        if scale:
            out[f"{label}__cc"] = np.rint(cc * scale).astype(np.uint16)  # cc = stored / ccscale, exactly
            assert np.array_equal(out[f"{label}__cc"].astype(np.float64) / float(scale), cc), label
        else:
            out[f"{label}__cc"] = cc.astype(np.float32) if np.all(cc == cc.astype(np.float32)) else cc
        out[f"{label}__ccscale"] = np.int64(max(scale, 1))
        out[f"{label}__ii"] = ii.astype(np.int32)
        out[f"{label}__kk"] = kk.astype(np.int16 if small else np.int32)
        out[f"{label}__solvable"] = np.bool_(solvable)
        out[f"{label}__strict"] = np.bool_(not solvable and certain_ret1(n, cc, ii, kk))
        out[f"{label}__aug"] = np.bool_(aug)
        out[f"{label}__dyn"] = np.int64(dyn)
        xs = {}
        for fp in (1, 2, 3):
            if not solvable and (fp == 2 or (fp == 3 and dyn == 2)):
                continue
            ret, x, y, secs = ref_solve(lib, n, cc, ii, kk, fp)
            if solvable:
                assert ret == 0 and np.array_equal(np.sort(x), np.arange(n)), (label, fp, ret)
                assert np.array_equal(x[y], np.arange(n)), (label, fp)
            xs[fp] = x
            if solvable and fp != 3:  # (FP_DYNAMIC is one of the two: v_3 would repeat v_dyn)
                vret, vx, vy, v = ref_duals(lib, n, cc, ii, kk, fp)
                assert vret == ret and np.array_equal(vx, x) and np.array_equal(vy, y), (label, fp)
                assert np.all(np.isfinite(v)), (label, fp)
                out[f"{label}__v_{fp}"] = v
            out[f"{label}__ret_{fp}"] = np.int64(ret)
            out[f"{label}__x_{fp}"] = x.astype(np.int16 if small else np.int32)
            out[f"{label}__y_{fp}"] = y.astype(np.int16 if small else np.int32)
            if times or n >= 257:
                print(f"{label} fp={fp} aug={aug} reference {secs * 1e3:.2f} ms")
        if 1 in xs and 2 in xs and not np.array_equal(xs[1], xs[2]):
            disagree += 1
        by_kind.setdefault(kind, []).append((label, n, aug))
    return out, by_kind, disagree


def same_as_committed(path, out):
    """Every key of the committed file equals what is about to be written (bits and dtype): stored cases never
    move.  True when the file holds nothing else either, so that it need not be rewritten."""
    if not path.exists():
        return False
    old = np.load(path, allow_pickle=False)
    for key in old.files:
        assert key in out and old[key].dtype == out[key].dtype and old[key].shape == np.shape(out[key]), key
        assert np.array_equal(old[key], out[key], equal_nan=old[key].dtype.kind == "f"), key
    print(f"{path.name}: {len(old.files)} committed keys equal to the regenerated ones")
    return set(old.files) == set(out)


def main():
    lib = lapmod_lib()
    lds_max = int(sys.argv[1]) if len(sys.argv) > 1 else 3395
    cases = stored_cases(lds_max)
    out, by_kind, disagree = records(lib, cases, times=False)
    out.update(labels=np.array([c[0] for c in cases]), lds_max_n=np.int64(lds_max))
    tie_aug = {}
    for _, n, aug in by_kind["tie"]:
        if n >= 63:
            tie_aug.setdefault(n, []).append(aug)
    for n, flags in tie_aug.items():
        assert 2 * sum(flags) >= len(flags), (n, flags)
    assert disagree >= 1
    assert out["empty_column__strict"] and out["infs_unsolvable0__strict"] and out["inf_col__strict"]
    path = HERE / "lapmod_cases.npz"
    if not same_as_committed(path, out):
        np.savez_compressed(path, **out)
    print(f"{len(cases)} cases, {disagree} with FP_1 != FP_2, {path.stat().st_size} bytes")

    # the long-row cases: a file of their own (both together would pass 1 MiB), read by the same loader
    cases = long_row_cases()
    assert not {c[0] for c in cases} & set(out["labels"].tolist())
    out, by_kind, disagree = records(lib, cases, times=True)
    out["labels"] = np.array([c[0] for c in cases])
    assert all(aug for _, _, aug in by_kind["long"]), by_kind["long"]
    print("augmentation reached by every solvable case:", [label for label, _, _ in by_kind["long"]])
    lengths = set()
    for label, n, cc, ii, kk, kind in cases:
        lengths |= set(np.diff(ii).tolist())
        assert not np.all(cc * 64 == np.floor(cc * 64)), label
    assert {64, 65, 128, 129, 193} <= lengths, sorted(lengths)
    print("row lengths include 64, 65, 128, 129, 193; no case has dyadic costs")
    picked = {label: int(out[f"{label}__dyn"]) for label, _, _ in by_kind["long"]}
    assert set(picked.values()) == {1, 2}, picked
    print("FP_DYNAMIC picks", picked)
    label, n, cc, ii, kk, _ = next(c for c in cases if c[0] == "dec_single193")
    above, far, free = arr_first_values(n, cc, ii, kk)
    assert (free > 0) == bool(out[f"{label}__aug"]), free  # the transcription ends ARR as the reference does
    assert above >= 1 and far >= 1, (above, far)
    out[f"{label}__arr_first_above"], out[f"{label}__arr_first_far"] = np.int64(above), np.int64(far)
    print(f"{label}: {above} ARR rows start above LARGE, {far} of them with the first entry below it at "
          f"position >= 64; {free} rows free after ARR")
    for label, _, _ in by_kind["unsolvable"]:
        assert out[f"{label}__strict"], label
        assert int(out[f"{label}__dyn"]) == 1 and f"{label}__ret_2" not in out, label
    print("unsolvable and strict:", [label for label, _, _ in by_kind["unsolvable"]])
    path = HERE / "lapmod_long_rows.npz"
    if not same_as_committed(path, out):
        np.savez_compressed(path, **out)
    print(f"{len(cases)} cases, {disagree} with FP_1 != FP_2, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
