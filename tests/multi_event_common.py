"""Shared by tests/test_gpu_multi_event_steps.py: integer-cost inputs on which relax steps with several tie events
are the rule, and a pure-Python restatement of the seeded solve that classifies every relax step of an input.

The restatement follows oracle/jv_oracle.c phase by phase (projection, row tightening, greedy matching, quality
gate, micro-ARR, shortest paths); only the inner loop of a relax step is written with numpy.  It is used for the
classes alone -- the expected (ret, x, y) and counters come from oracle.jv.seeded_raw, and the test asserts that the
two agree on the counters, so a classifier that drifts from the oracle names itself."""
import functools

import numpy as np

# The sizes are where the bitmap walk of the solver changes shape: one word, two words, one and two positions per
# thread (1024 / 1025), 64 words (2047 / 2048), four positions per thread with two words per lane (2049, 2080, 4096).
SIZES = (31, 33, 64, 65, 1024, 1025, 2047, 2048, 2049, 2080, 4096)
# (n, largest cost, seed kind, rng seed): every size with both cost ranges and both kinds of seed
CASES = [(n, cmax, kind, 1 + 4 * q + 2 * (cmax == 7) + (kind == "reduced"))
         for q, n in enumerate(SIZES) for cmax in (3, 7) for kind in ("zero", "reduced")]
CASES += [(64, 7, "zero", 45), (65, 7, "reduced", 27)]  # a free column that is the first of more than four events
# at two words per lane the costs above leave no multi-event step without an event inside the window (the many ties
# make the window wide): a wider range has every class there
CASES += [(2049, 255, "reduced", 50), (4096, 255, "zero", 50)]
RAGGED_SIZES = (65, 1025, 2049)  # one batch through the ragged entry point: three kernel configurations
TWO_WORDS_PER_LANE = 2049        # from this size on a lane of the bitmap walk holds two words


def classified(c):
    """The cases the Python classifier walks: all up to n = 1025, one per size and the wide-range ones above (its
    n x n array expressions take half a second at n = 4096)."""
    return c[0] <= 1025 or (c[1] >= 7 and c[2] == "reduced") or c[1] == 255

CLASSES = ("2 events", "3 events", "4 events", "5-8 events", "more than 8 events", "event inside the window",
           "no event inside the window",
           "free column first among more than four", "free column not first", "multi-event with lo+1 == hi",
           "multi-event with lo+2 == hi")


def make_input(n, cmax, kind, seed):
    rs = np.random.RandomState(1000 + seed)
    C = rs.randint(0, cmax + 1, (n, n)).astype(np.float64)
    if kind == "zero":
        return C, np.zeros(n), np.zeros(n)
    u = C.min(axis=1)
    return C, u, (C - u[:, None]).min(axis=0)


@functools.lru_cache(maxsize=None)
def case(k):
    return make_input(*CASES[k])


def classify(C, u_seed, v_seed, eps=1e-12):
    """Counts of the relax-step classes of the seeded solve of (C, u, v), and its (paths, finds, scan_steps).
    None where the solve does not take the shortest-path branch."""
    n = C.shape[0]
    u, v = u_seed.copy(), v_seed.copy()
    violated = ((u[:, None] + v[None, :]) - C > eps).any(axis=1)  # (a row without one now can get none later:
    for i in np.nonzero(violated)[0]:  # projection, Gauss-Seidel    the projection only lowers u and v)
        for j in np.nonzero((u[i] + v) - C[i] > eps)[0]:
            viol = (u[i] + v[j]) - C[i, j]
            if viol > eps:
                u[i] -= viol / 2.0
                v[j] -= viol / 2.0
    if (((C - u[:, None]) - v[None, :]) < -eps).any():
        return None
    u = (C - v[None, :]).min(axis=1)
    tight_eps = max(eps, 1e-9)
    tight = np.abs((C - u[:, None]) - v[None, :]) <= tight_eps
    x, y = np.full(n, -1), np.full(n, -1)
    for i in range(n):
        cand = np.nonzero(tight[i] & (y < 0))[0]
        if len(cand):
            x[i], y[cand[0]] = cand[0], i
    free_rows = np.nonzero(x < 0)[0]
    col_free = y < 0
    if int(tight.sum()) < 1.2 * n or len(free_rows) == 0:
        return None
    for i in free_rows:  # micro-ARR
        r = (C[i] - u[i]) - v
        j1 = int(np.argmin(r))
        m1 = r[j1]
        m2 = np.delete(r, j1).min() if n > 1 else np.inf
        if m2 - m1 > tight_eps and col_free[j1]:
            v[j1] += m2 - m1
    counts = dict.fromkeys(CLASSES, 0)
    paths = finds = steps = 0
    for start in free_rows:
        order = np.arange(n)
        pred = np.full(n, start)
        dist = C[start] - v
        lo = hi = ready = 0
        target = -1
        paths += 1
        while target < 0:
            if lo == hi:
                ready = lo
                hi = lo + 1
                best = dist[order[lo]]
                # the swap sequence is observable: keep it serial, over the positions that can swap at all (those
                # not above the running minimum of what lies before them; swaps never touch a position further on)
                d = dist[order[lo + 1:]]
                before = np.minimum.accumulate(np.concatenate(([best], d)))[:-1]
                for k in lo + 1 + np.nonzero(d <= before)[0]:
                    j = order[k]
                    if dist[j] <= best:
                        if dist[j] < best:
                            hi, best = lo, dist[j]
                        order[k], order[hi] = order[hi], j
                        hi += 1
                finds += 1
                for k in range(lo, hi):
                    if y[order[k]] < 0:
                        target = order[k]
            while target < 0 and lo != hi:
                j = order[lo]
                lo += 1
                i, level = y[j], dist[j]
                h = (C[i, j] - v[j]) - level
                steps += 1
                cols = order[hi:]
                cand = (C[i, cols] - v[cols]) - h
                imp = cand < dist[cols]
                ev_pos = hi + np.nonzero(imp & (cand == level))[0]  # exact on the pre-loop order (positions above
                free_ev = [p for p in ev_pos if y[order[p]] < 0]    # the one examined are never touched)
                if free_ev:
                    upto = free_ev[0]  # the serial loop returns here: later columns stay unrelaxed
                    sel = np.arange(hi, upto + 1)
                    m = imp[:upto + 1 - hi]
                else:
                    sel, m = np.arange(hi, n), imp
                dist[order[sel][m]] = cand[:len(sel)][m]
                pred[order[sel][m]] = i
                cnt = len(ev_pos)
                if cnt >= 2:
                    if free_ev:
                        if free_ev[0] == ev_pos[0] and cnt > 4:
                            counts["free column first among more than four"] += 1
                        if free_ev[0] != ev_pos[0]:
                            counts["free column not first"] += 1
                    else:
                        name = {2: "2 events", 3: "3 events", 4: "4 events"}.get(cnt, "5-8 events" if cnt <= 8 else
                                                                                 "more than 8 events")
                        counts[name] += 1
                        counts["event inside the window" if ev_pos[0] < hi + cnt else "no event inside the window"] += 1
                    if lo == hi:  # (lo is already past the head: the head sat at hi - 1)
                        counts["multi-event with lo+1 == hi"] += 1
                    if lo + 1 == hi:
                        counts["multi-event with lo+2 == hi"] += 1
                if free_ev:
                    target = order[free_ev[0]]
                    lo -= 1  # the early return leaves lo on the head
                    break
                for p in ev_pos:
                    order[p], order[hi] = order[hi], order[p]
                    hi += 1
        level = dist[order[lo]]
        for k in range(ready):
            v[order[k]] += dist[order[k]] - level
        j, i = target, -1
        while i != start:
            i = pred[j]
            y[j] = i
            j, x[i] = x[i], j
    return counts, (paths, finds, steps)


def make_pack(mats):
    """A packed RaggedPack of the matrices, NaN in every cell that belongs to no instance."""
    import torch

    from gnn.features import RaggedPack
    sizes = [m.shape[0] for m in mats]
    offsets, total = [], 1  # one leading NaN: odd element offsets, 8-byte alignment only
    for n in sizes:
        offsets.append(total)
        total += n * n + 1
    buf = np.full(total, np.nan)
    for m, o, n in zip(mats, offsets, sizes):
        buf[o:o + n * n] = m.ravel()
    return RaggedPack(torch.from_numpy(buf).cuda(), torch.tensor(offsets, dtype=torch.int64).cuda(),
                      torch.tensor(sizes, dtype=torch.int32).cuda(), None, None, 0, max(sizes), sizes)


def padded_seeds(seeds, N):
    import torch
    out = np.full((2, len(seeds), N), np.nan)
    for b, (u, v) in enumerate(seeds):
        out[0, b, :len(u)], out[1, b, :len(v)] = u, v
    t = torch.from_numpy(out).cuda()
    return t[0].contiguous(), t[1].contiguous()
