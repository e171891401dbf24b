"""A NumPy model of the ragged oracle-duals driver (lapwarm_oracle_duals_ragged) and of the uniform driver it
must agree with, instance by instance; the chain instance whose Jacobi sweeps outlast the budget; a small exact
assignment solver for matchings on the host (shared by test_oracle_duals_ragged_host.py and
test_gpu_oracle_duals_ragged.py)."""
import numpy as np

REPLAY_MAX_N = 2048  # kOracleReplayMaxN
RUNNING, DONE, REPLAY, NEGATIVE_CYCLE = 0, 100, 101, 1
EMPTY = 6            # kOracleEmpty: the ret code of an instance a ragged call treats as empty


def chain_instance(n):
    """C = n everywhere, 0 on the diagonal, -1 right of it; with the identity matching column j is reached from
    column 0 over j edges of weight -1, one more per Jacobi sweep: v = 0, -1, ..., -(n - 1) after n - 1 updating
    sweeps, so the n - 1 sweeps of the budget do not settle it."""
    C = np.full((n, n), float(n))
    i = np.arange(n)
    C[i, i] = 0.0
    C[i[:-1], i[:-1] + 1] = -1.0
    return C


def hungarian(C):
    """An optimal assignment of a small square matrix, row -> column (shortest augmenting paths, O(n^3))."""
    n = C.shape[0]
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    p, way = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(n + 1, np.inf)
        used = np.zeros(n + 1, dtype=bool)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], np.inf, 0
            for j in range(1, n + 1):
                if not used[j]:
                    cur = C[i0 - 1, j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(n + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    x = np.empty(n, dtype=np.int64)
    x[p[1:] - 1] = np.arange(n)
    return x


class Instance:
    """The per-instance state of the sweep kernels: v, the predecessor rows, the sweeps made, whether the last
    sweep changed a column (the next active list is not empty), and the status."""

    def __init__(self, C, x):
        self.C, self.x, self.n = np.asarray(C, dtype=np.float64), np.asarray(x), C.shape[0]
        self.W = self.C - self.C[np.arange(self.n), self.x][:, None]
        self.v = np.zeros(self.n)
        self.pred = np.full(self.n, -1)
        self.sweeps, self.active, self.status = 0, True, RUNNING

    def sweep(self, s):
        """Sweep s of the batch.  The instance's own budget: none once it has made n - 1."""
        if self.status != RUNNING or s >= self.n - 1:
            return
        if not self.active:
            self.status = DONE
            return
        cand = self.v[self.x][:, None] + self.W
        arg = cand.argmin(axis=0)  # ties: the smallest row
        m = cand[arg, np.arange(self.n)]
        changed = self.v > m
        self.v = np.where(changed, m, self.v)
        self.pred[changed] = arg[changed]
        self.sweeps = s + 1
        self.active = bool(changed.any())

    def has_cycle(self):
        nxt = np.where(self.pred < 0, -1, self.x[np.maximum(self.pred, 0)])
        for j in range(self.n):
            k = j
            for _ in range(self.n + 1):
                if k < 0:
                    break
                k = nxt[k]
            if k >= 0:
                return True
        return False

    def check(self, last):
        """-> does the instance go on sweeping"""
        if self.status != RUNNING:
            return False
        if not self.active:
            self.status = DONE
            return False
        if self.has_cycle() or last:
            self.status = REPLAY if self.n <= REPLAY_MAX_N else NEGATIVE_CYCLE
            return False
        return True

    def result(self):
        return self.v.copy(), self.sweeps, self.status == REPLAY


def run_driver(instances, ragged, max_s=None):
    """The host loop: chunks of 4, 8, 16, then 32 sweeps, a check after each.  Uniform (one size): the last check
    comes with `last`.  Ragged: the schedule runs to the largest budget and every instance is checked with its own
    last_b = (s >= n_b - 1), or with the host's `last` where the schedule ends before its own budget (`max_s`: a
    host budget below the largest instance's).  Returns the number of checks (host synchronisations, the last one
    apart)."""
    max_s = max(t.n for t in instances) - 1 if max_s is None else max_s
    assert ragged or len({t.n for t in instances}) == 1
    s, chunk, checks = 0, 4, 0
    while True:
        for _ in range(min(chunk, max_s - s)):
            for t in instances:
                t.sweep(s)
            s += 1
        last = s >= max_s
        checks += 1
        running = [t.check(last or s >= t.n - 1 if ragged else last) for t in instances]
        if last or not any(running):
            return checks
        chunk = min(32, chunk * 2)


def model_alone(C, x):
    t = Instance(C, x)
    run_driver([t], ragged=False)
    return t.result()


def model_ragged(pairs):
    ts = [Instance(C, x) for C, x in pairs]
    run_driver(ts, ragged=True)
    return [t.result() for t in ts]
