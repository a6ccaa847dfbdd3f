"""TEST INFRASTRUCTURE -- the float64 NumPy restatement of gsttaco_mel_dtw (csrc/dtw.hip; the contract in include/gsttaco.h) and the case
table its tests share.  tests/test_gpu_dtw.py compares the device against ``dtw_reference``; tests/test_dtw_cases.py pins the
restatement and the conditioning of every case on the CPU.

The restatement: features = clip(x) (to the normalisation's range) in double, times rows 1..n_ceps of the orthonormal DCT-II
(``evaluate.dct_basis``) or taken as they are (n_ceps 0), times ``evaluate.mcd_scale``; C(i,j) the Euclidean distance;
D(i,j) = C(i,j) + min over the predecessors, swept one anti-diagonal at a time; ties: the diagonal, replaced by up (i-1,j) only if
strictly smaller, then by left (i,j-1) only if strictly smaller than the best so far; the path is walked back by the same choices.
"""
import collections
import functools

import numpy as np

from gst_tacotron_amd import evaluate, hparams, synthetic

RTOL = 1e-9     # both sides are double and differ by FMA contraction and summation order over at most 80 channels: ~1e-14 of the feature
                # magnitude, amplified at most ~1e3 by cancellation where y is a warped copy of x; two decades of margin, and an fp32
                # accumulator or fp32 features miss it by six
MAX_STEP = 1100     # what the test contexts set: above the 1024 threads of the sweep's workgroup

# shapes: (Lx, Ly) per row; Tx / Ty: the padded sizes (None = the largest length); kind: noise | warp | identical | beyond | unit
Case = collections.namedtuple("Case", "name shapes kind mel n_ceps max_abs Tx Ty seed max_step")


def _case(name, shapes, kind, mel=80, n_ceps=13, max_abs=4.0, Tx=None, Ty=None, seed=0, max_step=MAX_STEP):
    Tx = Tx or max(max(s[0] for s in shapes), 1)
    Ty = Ty or max(max(s[1] for s in shapes), 1)
    return Case(name, tuple(shapes), kind, mel, n_ceps, max_abs, Tx, Ty, seed, max_step)


RAGGED = ((37, 53), (0, 9), (12, 0), (20, 20))
CASES = collections.OrderedDict((c.name, c) for c in (
    _case("edges_noise", [(1, 1), (1, 7), (5, 1)], "noise", seed=1),
    _case("edges_warp_tiny_mel", [(1, 1), (1, 7), (5, 1)], "warp", mel=16, n_ceps=15, seed=2),
    _case("generic_noise", [(37, 53)], "noise", seed=3),
    _case("generic_warp", [(37, 53)], "warp", seed=4),
    _case("generic_noise_channels", [(37, 53)], "noise", n_ceps=0, seed=5),
    _case("generic_warp_all_ceps", [(37, 53)], "warp", n_ceps=79, seed=6),
    _case("generic_noise_tiny_mel", [(37, 53)], "noise", mel=16, n_ceps=13, seed=7),
    _case("generic_warp_tiny_mel_channels", [(37, 53)], "warp", mel=16, n_ceps=0, seed=8),
    _case("wave_edge_noise", [(64, 65), (65, 64)], "noise", seed=9),
    _case("wave_edge_warp", [(64, 65), (65, 64)], "warp", seed=10),
    _case("several_waves_noise", [(130, 97)], "noise", seed=11),
    _case("several_waves_warp", [(130, 97)], "warp", mel=16, n_ceps=15, seed=12),
    _case("wide", [(3, 1100)], "noise", seed=13),
    _case("tall", [(1100, 3)], "noise", seed=14),
    _case("wide_warp", [(3, 1100)], "warp", mel=16, n_ceps=13, seed=15),
    _case("ragged_noise", RAGGED, "noise", Tx=40, Ty=56, seed=16),
    _case("ragged_warp", RAGGED, "warp", n_ceps=0, Tx=40, Ty=56, seed=17),
    _case("identical", [(37, 37)], "identical", seed=18),
    _case("identical_channels", [(37, 37), (5, 5)], "identical", mel=16, n_ceps=0, seed=19),
    _case("beyond_range", [(37, 53)], "beyond", seed=20),
    _case("unit_range", [(37, 53)], "unit", max_abs=0.0, seed=21),
    _case("unit_range_warp", [(37, 53)], "unit_warp", max_abs=0.0, n_ceps=0, mel=16, seed=22),
    # (the rolling diagonals of 2000 columns need 72 000 bytes of LDS: above the 64 KiB a launch gets without asking)
    _case("lds_above_64k", [(3, 2000)], "noise", mel=16, n_ceps=13, seed=23, max_step=2000),
))
NAMES = list(CASES)


def case_hp(case):
    """The hyper parameters of a case's context: the shipped ones (Mel_Dim 80) or ``synthetic.tiny_hp``'s, Max_Step and Max_Abs_Mel set."""
    hp = hparams.load_hp() if case.mel == 80 else synthetic.tiny_hp(max_step=case.max_step)
    hp["Max_Step"] = case.max_step
    hp["Sound"]["Max_Abs_Mel"] = case.max_abs
    assert hp["Sound"]["Mel_Dim"] == case.mel
    return hp


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(x [B, Tx, mel], x_len, y [B, Ty, mel], y_len) float32 / int32, every element finite (the frames beyond a length hold ordinary
    values here, so that the same arrays serve the NULL- and clipped-length calls; ``nan_padded`` fills them with NaN).  Read-only."""
    c = CASES[name]
    rng = np.random.default_rng(1000 + c.seed)
    B = len(c.shapes)
    lo, hi = (-c.max_abs, c.max_abs) if c.max_abs > 0 else (0.0, 1.0)

    def noise(shape):
        if c.kind.startswith("unit"):
            v = rng.normal(0.5, 0.3, size=shape)
        else:
            v = rng.normal(0.0, 1.5, size=shape) * (2.0 if c.kind == "beyond" else 1.0)
        v = v.astype(np.float32)
        return v if c.kind == "beyond" else np.clip(v, np.float32(lo), np.float32(hi))

    x, y = noise((B, c.Tx, c.mel)), noise((B, c.Ty, c.mel))
    for b, (Lx, Ly) in enumerate(c.shapes):
        if c.kind == "identical":
            y[b, :Ly] = x[b, :Lx]
        elif c.kind.endswith("warp") and Lx and Ly:
            idx = np.sort(rng.integers(0, Lx, size=Ly))
            w = x[b, idx].astype(np.float64) + rng.normal(0.0, 0.01, size=(Ly, c.mel))
            y[b, :Ly] = np.clip(w.astype(np.float32), np.float32(lo), np.float32(hi))
    if c.kind == "beyond":
        assert (np.abs(x) > c.max_abs).mean() > 0.05 and (np.abs(y) > c.max_abs).mean() > 0.05
    out = (x, np.array([s[0] for s in c.shapes], np.int32), y, np.array([s[1] for s in c.shapes], np.int32))
    for a in out:
        a.setflags(write=False)
    return out


def nan_padded(a, lengths):
    """A writable copy of ``a`` [B, T, .] with NaN in every frame at or beyond its row's length."""
    a = np.array(a)
    for b, n in enumerate(lengths):
        a[b, max(int(n), 0):] = np.nan
    return a


# ---------------------------------------------------------------------------------------------------- the restatement
def features(frames, hp, n_ceps, dtype=np.float64):
    """[T, mel] float32 -> [T, F] in ``dtype``: clip, widen, (DCT-II rows 1..n_ceps,) scale."""
    lo, hi = evaluate.mel_range(hp)
    v = np.clip(np.asarray(frames, np.float32), np.float32(lo), np.float32(hi)).astype(dtype)
    if n_ceps:
        # (not a matmul: BLAS sums a row in an order that depends on how many rows there are, and equal frames must give equal features)
        v = (v[:, None, :] * evaluate.dct_basis(n_ceps, v.shape[-1]).astype(dtype)[None, :, :]).sum(axis=-1)
    return v * dtype(evaluate.mcd_scale(hp))


def local_cost(f, g):
    """C [Lx, Ly]: Euclidean distances of the rows of f and g, in their dtype."""
    d = f[:, None, :] - g[None, :, :]
    return np.sqrt((d * d).sum(axis=-1))


def dtw_table(C):
    """(D, direction) of a local-cost matrix [Lx >= 1, Ly >= 1], one vectorised step per anti-diagonal.  direction: 0 diagonal, 1 up
    (i-1, j), 2 left (i, j-1); cell (0, 0) holds 0."""
    Lx, Ly = C.shape
    inf = C.dtype.type(np.inf)
    D = np.full((Lx + 1, Ly + 1), inf, C.dtype)            # D[i + 1, j + 1] = D(i, j); row / column 0: no such predecessor
    dirs = np.zeros((Lx, Ly), np.int8)
    for d in range(Lx + Ly - 1):
        j = np.arange(max(0, d - (Lx - 1)), min(d, Ly - 1) + 1)
        i = d - j
        best, pick = D[i, j].copy(), np.zeros(j.shape, np.int8)
        up, left = D[i, j + 1], D[i + 1, j]
        m = up < best
        best[m], pick[m] = up[m], 1
        m = left < best
        best[m], pick[m] = left[m], 2
        if d == 0:
            best[:] = 0
        D[i + 1, j + 1] = C[i, j] + best
        dirs[i, j] = pick
    return D[1:, 1:], dirs


def walk_back(dirs):
    """The cells [(i, j)] from (0, 0) to the last one along the chosen predecessors."""
    i, j = dirs.shape[0] - 1, dirs.shape[1] - 1
    cells = [(i, j)]
    while i or j:
        k = dirs[i, j]
        i, j = i - (k != 2), j - (k != 1)
        cells.append((i, j))
    return cells[::-1]


def dtw_reference(x, x_len, y, y_len, hp, n_ceps, dtype=np.float64, with_tables=False):
    """(cost [B] in ``dtype``, path_len int32 [B], path int32 [B, Tx + Ty - 1, 2] with -1 beyond the length) of x [B, Tx, mel] against
    y [B, Ty, mel]; lengths None = all frames, clipped to [0, T] otherwise.  ``with_tables``: also the lists of C and D per row (None
    for a row without frames)."""
    x, y = np.asarray(x), np.asarray(y)
    B, Tx, Ty = x.shape[0], x.shape[1], y.shape[1]
    cost, n, path = np.zeros(B, dtype), np.zeros(B, np.int32), np.full((B, Tx + Ty - 1, 2), -1, np.int32)
    Cs, Ds = [], []
    for b in range(B):
        Lx = Tx if x_len is None else int(np.clip(x_len[b], 0, Tx))
        Ly = Ty if y_len is None else int(np.clip(y_len[b], 0, Ty))
        if Lx == 0 or Ly == 0:
            Cs.append(None), Ds.append(None)
            continue
        C = local_cost(features(x[b, :Lx], hp, n_ceps, dtype), features(y[b, :Ly], hp, n_ceps, dtype))
        D, dirs = dtw_table(C)
        cells = walk_back(dirs)
        cost[b], n[b] = D[-1, -1], len(cells)
        path[b, :len(cells)] = cells
        Cs.append(C), Ds.append(D)
    return (cost, n, path, Cs, Ds) if with_tables else (cost, n, path)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """``dtw_reference(..., with_tables=True)`` of a case, computed once."""
    c = CASES[name]
    x, xl, y, yl = case_inputs(name)
    return dtw_reference(x, xl, y, yl, case_hp(c), c.n_ceps, with_tables=True)


def brute_force(C):
    """(cost, cells) of a small C by plain top-down recursion over the cells with the tie rule -- no table, no anti-diagonals."""
    def best(i, j):
        if i == 0 and j == 0:
            return C[0, 0], [(0, 0)]
        cands = []
        if i > 0 and j > 0:
            cands.append(best(i - 1, j - 1))
        if i > 0:
            cands.append(best(i - 1, j))
        if j > 0:
            cands.append(best(i, j - 1))
        pick = cands[0]
        for c in cands[1:]:
            if c[0] < pick[0]:
                pick = c
        return C[i, j] + pick[0], pick[1] + [(i, j)]
    return best(C.shape[0] - 1, C.shape[1] - 1)


def path_is_valid(cells, Lx, Ly):
    """A warping path: from (0, 0) to (Lx - 1, Ly - 1) by steps (1, 1), (1, 0) or (0, 1)."""
    cells = [tuple(int(v) for v in c) for c in cells]
    if not cells or cells[0] != (0, 0) or cells[-1] != (Lx - 1, Ly - 1):
        return False
    return all((c[0] - p[0], c[1] - p[1]) in ((1, 1), (1, 0), (0, 1)) for p, c in zip(cells, cells[1:]))


def path_margin(C, D, cells):
    """The smallest relative gap, over the path's cells with more than one predecessor, between the chosen predecessor's D and the
    runner-up's: (runner-up - chosen) / runner-up.  inf when no cell has a choice."""
    worst = np.inf
    for (pi, pj), (i, j) in zip(cells, cells[1:]):
        if i == 0 or j == 0:
            continue
        cands = {(i - 1, j - 1): D[i - 1, j - 1], (i - 1, j): D[i - 1, j], (i, j - 1): D[i, j - 1]}
        chosen = cands.pop((pi, pj))
        second = min(cands.values())
        worst = min(worst, float((second - chosen) / second) if second > 0 else 0.0)
    return worst
