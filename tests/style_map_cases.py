"""The float64 restatement of gsttaco_style_affinities and gsttaco_style_map (include/gsttaco.h), written from the contract there and
not from csrc/tsne.hip, and the case table both test files share: tests/test_style_map_cases.py admits the cases on the CPU (float64
against np.longdouble: every decision decided, the two precisions within RTOL / 16), tests/test_gpu_style_map.py runs them on the GPU.

The affinity cases name the smallest shapes at which the kernels can go wrong: N around a wavefront (63 / 64 / 65), around a tile at
the shipped embedding width (255 / 257 x 256), more points than the search's workgroup has lanes and than the pair kernel's LDS tile
holds (1030), duplicates and an outlier (beta at both ends of the search), a perplexity below a point's number of duplicates (all 200
rounds), a row stride wider than the embedding.  The descent is chaotic -- float64 and long double differ by 3e-14 of max|y| after 10
steps from t = 0 of ``blobs120`` and by more than max|y| itself after 60 -- so the descent cases are at most 10 steps from states of
the restatement's own 1000-step run, and longer runs are judged by what they must achieve (``BLOBS_KL``, nearest-neighbour purity),
not value by value.
"""
import functools

import numpy as np

RTOL = 1e-9                     # device against float64; the admission holds float64 against long double to RTOL / 16
MARGIN = 1e-9                   # by how much every decision falls (Hd in nats; |g| relative to the largest)
SEARCH_TOL, SEARCH_ROUNDS = 1e-5, 200
DEFAULTS = dict(exaggeration=12.0, stop_lying_iter=250, mom_switch_iter=250, momentum=0.5, final_momentum=0.8, eta=200.0)
# KL of the restatement's 1000-step run of ``blobs120`` at the defaults, seeds 0 .. 3, as first computed.  A run of 1000 steps is one of
# many equally valid trajectories (another exp in the last bit gives another), so these are a yardstick of what a good run reaches --
# tests/test_style_map_cases.py holds a rerun within a factor 1.25 of them -- and not values to reproduce.
BLOBS_KL = (0.7205017, 0.7318514, 0.7067318, 0.7219385)


def _frozen(a):
    a = np.array(a, order="C")
    a.setflags(write=False)
    return a


def default_init(n, seed=0):
    """y at t = 0 where no ``init`` is given: drawn on the host."""
    return np.random.default_rng(seed).standard_normal((n, 2)) * 1e-4


# ------------------------------------------------------------------------------------------------ the affinities, restated
def distances(x, dtype=np.float64):
    """d_ij = sum_k (x_ik - x_jk)^2: one accumulator per pair, ascending k, the square and the sum each rounded."""
    xd = np.asarray(x).astype(dtype)
    d = np.zeros((xd.shape[0], xd.shape[0]), dtype)
    for k in range(xd.shape[1]):
        df = xd[:, None, k] - xd[None, :, k]
        d = d + df * df
    return d


def affinities_reference(x, perplexity, dtype=np.float64):
    """Returns dict(p, cond, beta, search_iters, margin): ``margin`` is the smallest amount (nats) by which a decision of the search fell
    -- Hd against 0 where its sign was used, |Hd| against SEARCH_TOL in every round."""
    d = distances(x, dtype)
    N = d.shape[0]
    off = ~np.eye(N, dtype=bool)
    delta = np.where(off, d - np.where(off, d, np.inf).min(axis=1)[:, None], dtype(0))
    target = np.log(dtype(np.float32(perplexity)))
    beta = np.ones(N, dtype)
    lo, hi = np.full(N, -np.inf, dtype), np.full(N, np.inf, dtype)
    rounds = np.zeros(N, np.int32)
    active = np.ones(N, bool)
    margin = np.inf

    def weights(rows):
        w = np.where(off[rows], np.exp(-beta[rows, None] * delta[rows]), dtype(0))
        return w, w.sum(axis=1)

    w, s = weights(np.arange(N))
    for it in range(SEARCH_ROUNDS + 1):
        rows = np.nonzero(active)[0]
        if rows.size == 0:
            break
        wr, sr = weights(rows)
        w[rows], s[rows] = wr, sr
        if it == SEARCH_ROUNDS:                                         # the weights once more at the beta 200 undecided rounds left
            break
        t = np.where(off[rows], delta[rows] * wr, dtype(0)).sum(axis=1)
        hd = np.log(sr) + beta[rows] * t / sr - target
        rounds[rows] += 1
        margin = min(margin, float(np.abs(np.abs(hd) - SEARCH_TOL).min()))
        done = np.abs(hd) < SEARCH_TOL
        up, down = rows[~done & (hd > 0)], rows[~done & ~(hd > 0)]
        lo[up] = beta[up]
        beta[up] = np.where(hi[up] == np.inf, beta[up] * 2, (beta[up] + hi[up]) / 2)
        hi[down] = beta[down]
        beta[down] = np.where(lo[down] == -np.inf, beta[down] / 2, (beta[down] + lo[down]) / 2)
        active[rows[done]] = False
    cond = w / s[:, None]
    p = (cond + cond.T) / dtype(2 * N)
    p[~off] = 0
    return dict(p=p, cond=cond, beta=beta, search_iters=rounds, margin=margin)


# ------------------------------------------------------------------------------------------------ the descent, restated
def pair_terms(p, y):
    """n (zero diagonal), Z and the differences y_i - y_j."""
    diff = y[:, None, :] - y[None, :, :]
    n = 1 / (1 + (diff[:, :, 0] * diff[:, :, 0] + diff[:, :, 1] * diff[:, :, 1]))
    np.fill_diagonal(n, 0)
    return n, n.sum(axis=1).sum(), diff


def descent_reference(p, y, velocity, gains, first_iter, iters, exaggeration=12.0, stop_lying_iter=250, mom_switch_iter=250, momentum=0.5,
                      final_momentum=0.8, eta=200.0, dtype=np.float64, snapshots=()):
    """``iters`` steps from the given state.  Returns dict(y, velocity, gains, iter, decisions, g_ratio, snaps): ``decisions`` are the
    sign(g) != sign(velocity) outcomes of every step, ``g_ratio`` the smallest min|g| / max|g| of a step, ``snaps`` the states at the
    steps named in ``snapshots``.  The float parameters are the float32 values the C ABI carries."""
    f = lambda v: dtype(np.float32(v))
    p, y, velocity, gains = (np.array(a, dtype) for a in (p, y, velocity, gains))
    N = y.shape[0]
    decisions, g_ratio, snaps = [], np.inf, {}
    for t in range(first_iter, first_iter + iters):
        if t in snapshots:
            snaps[t] = (y.copy(), velocity.copy(), gains.copy())
        e = f(exaggeration) if t < stop_lying_iter else dtype(1)
        m = f(momentum) if t < mom_switch_iter else f(final_momentum)
        n, Z, diff = pair_terms(p, y)
        A = ((p * n)[:, :, None] * diff).sum(axis=1)
        B = ((n * n)[:, :, None] * diff).sum(axis=1)
        g = e * A - B / Z
        differ = np.sign(g) != np.sign(velocity)
        decisions.append(differ)
        g_ratio = min(g_ratio, float(np.abs(g).min() / np.abs(g).max()))
        gains = np.maximum(np.where(differ, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
        velocity = m * velocity - f(eta) * gains * g
        y = y + velocity
        y = y - y.sum(axis=0) / dtype(N)
    if first_iter + iters in snapshots:
        snaps[first_iter + iters] = (y.copy(), velocity.copy(), gains.copy())
    return dict(y=y, velocity=velocity, gains=gains, iter=first_iter + iters, decisions=np.array(decisions), g_ratio=g_ratio, snaps=snaps)


def kl_reference(p, y, dtype=np.float64):
    p, y = np.asarray(p, dtype), np.asarray(y, dtype)
    n, Z, _ = pair_terms(p, y)
    m = p > 0
    return float((p[m] * np.log(p[m] / (n[m] / Z))).sum())


def purity(y, labels):
    """The share of points whose nearest neighbour in the map carries their own label."""
    y = np.asarray(y, np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return float((np.asarray(labels)[d.argmin(axis=1)] == labels).mean())


# ------------------------------------------------------------------------------------------------ the data
def _normal(seed, n, d, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((n, d)) * scale).astype(np.float32)


def _blobs120():
    rng = np.random.default_rng(120)
    centres = rng.normal(0.0, 4.0, (3, 16))                             # N(0, 16)
    return np.concatenate([c + rng.standard_normal((40, 16)) for c in centres]).astype(np.float32)


BLOBS_LABELS = _frozen(np.repeat(np.arange(3), 40))


def _dups_outlier():
    x = _normal(33, 33, 8)
    x[1] = x[2] = x[0]                                                  # three identical rows
    x[32] = 0
    x[32, 3] = 100.0                                                    # one row 100 units away
    return x


def _three_duplicates():
    x = _normal(12, 12, 4)
    x[1] = x[2] = x[3] = x[0]                                           # rows 0 .. 3 each have three duplicates: H >= log 3 > log 2.5
    return x


class AffinityCase:
    def __init__(self, name, x, perplexity, D=None):
        self.name, self.perplexity = name, float(perplexity)
        self.wide = _frozen(x)                                          # what lies in memory: [N, ldx]
        self.D = int(D if D is not None else x.shape[1])
        self.ldx = int(x.shape[1])
        self.x = self.wide[:, :self.D]
        self.N = int(x.shape[0])


AFFINITY_CASES = {c.name: c for c in (
    AffinityCase("n3", _normal(3, 3, 2), 1.5),
    AffinityCase("n7_d1", _normal(7, 7, 1), 2.0),
    AffinityCase("n63", _normal(63, 63, 3), 5.0),
    AffinityCase("n64", _normal(64, 64, 3), 5.0),
    AffinityCase("n65", _normal(65, 65, 3), 5.0),
    AffinityCase("n255_d256", _normal(255, 255, 256, 0.3), 30.0),
    AffinityCase("n257_d256", _normal(257, 257, 256, 0.3), 30.0),
    AffinityCase("dups_outlier", _dups_outlier(), 4.0),
    AffinityCase("three_duplicates", _three_duplicates(), 2.5),
    AffinityCase("wide_rows", _normal(20, 20, 9), 3.0, D=6),
    AffinityCase("n1030", _normal(1030, 1030, 5), 10.0),
    AffinityCase("blobs120", _blobs120(), 5.0),
)}
AFFINITY_NAMES = tuple(AFFINITY_CASES)


@functools.lru_cache(maxsize=None)
def affinity_reference(name, dtype=np.float64):
    c = AFFINITY_CASES[name]
    r = affinities_reference(c.x, c.perplexity, dtype)
    return {k: _frozen(v) if isinstance(v, np.ndarray) else v for k, v in r.items()}


# ------------------------------------------------------------------------------------------------ the descent cases
RUNS = {        # name -> (affinity case, seed of the init, schedule): the 1000-step runs the descent cases start from
    "blobs120": ("blobs120", 0, {}),
    "dups_outlier": ("dups_outlier", 0, {}),
    "early_switches": ("blobs120", 1, dict(stop_lying_iter=3, mom_switch_iter=4)),
}
STARTS = (0, 245, 500, 990)


@functools.lru_cache(maxsize=None)
def run_states(run):
    """The float64 states (y, velocity, gains) of a run at STARTS and at 1000."""
    aff, seed, schedule = RUNS[run]
    p = affinity_reference(aff)["p"]
    N = p.shape[0]
    r = descent_reference(p, default_init(N, seed), np.zeros((N, 2)), np.ones((N, 2)), 0, 1000, snapshots=STARTS + (1000,), **schedule)
    return {t: tuple(_frozen(a) for a in s) for t, s in r["snaps"].items()}


@functools.lru_cache(maxsize=None)
def blobs_run(seed):
    """The restatement's 1000 steps of ``blobs120`` at the defaults from ``default_init(120, seed)``: (y, kl)."""
    p = affinity_reference("blobs120")["p"]
    if seed == RUNS["blobs120"][1]:
        y = run_states("blobs120")[1000][0]
    else:
        y = descent_reference(p, default_init(120, seed), np.zeros((120, 2)), np.ones((120, 2)), 0, 1000)["y"]
    return _frozen(y), kl_reference(p, y)


class DescentCase:
    def __init__(self, name, affinity, state, first_iter, iters, schedule=None, kl_only=False):
        self.name, self.affinity, self._state, self.first_iter, self.iters = name, affinity, state, first_iter, iters
        self.schedule = dict(schedule or {})
        self.kl_only = kl_only

    @property
    def p(self):
        return affinity_reference(self.affinity)["p"]

    @property
    def state(self):
        return self._state()


def _pinned_gains():
    y, v, g = run_states("blobs120")[500]
    return y, v, _frozen(np.full_like(g, 0.011))                        # 0.011 * 0.8 < 0.01 wherever the signs agree


def _first_state():
    p = affinity_reference("n1030")["p"]
    return _frozen(default_init(p.shape[0], 5)), _frozen(np.zeros((p.shape[0], 2))), _frozen(np.ones((p.shape[0], 2)))


def _descent_cases():
    cases = []
    for run in ("blobs120", "dups_outlier"):
        for t in STARTS:
            for k in (1, 5, 10):
                cases.append(DescentCase("%s_from_%d_steps_%d" % (run, t, k), RUNS[run][0], functools.partial(lambda r, t: run_states(r)[t], run, t),
                                         t, k, RUNS[run][2]))
    for t in (0, 245):
        cases.append(DescentCase("early_switches_from_%d_steps_10" % t, "blobs120", functools.partial(lambda t: run_states("early_switches")[t], t),
                                 t, 10, RUNS["early_switches"][2]))
    cases.append(DescentCase("pinned_gains", "blobs120", _pinned_gains, 500, 3))
    cases.append(DescentCase("n1030_from_0_steps_5", "n1030", _first_state, 0, 5))      # more points than one LDS tile of the map holds
    cases.append(DescentCase("kl_only", "blobs120", lambda: run_states("blobs120")[1000], 1000, 0, kl_only=True))
    return {c.name: c for c in cases}


DESCENT_CASES = _descent_cases()
DESCENT_NAMES = tuple(DESCENT_CASES)


@functools.lru_cache(maxsize=None)
def descent_case_reference(name, dtype=np.float64):
    c = DESCENT_CASES[name]
    y, v, g = c.state
    r = descent_reference(c.p, y, v, g, c.first_iter, c.iters, dtype=dtype, **c.schedule)
    r["kl"] = kl_reference(c.p, r["y"], dtype)
    return {k: _frozen(a) if isinstance(a, np.ndarray) else a for k, a in r.items()}
