"""The float64 restatement of gsttaco_pitch and gsttaco_pitch_errors (include/gsttaco.h), written from the contract there and not from
csrc/pitch.hip, and the case table both test files share: tests/test_pitch_cases.py checks on the CPU that the restatement gives the
known answers and that every case is well conditioned, tests/test_gpu_pitch.py runs the cases on the GPU.

The tracker cases use small windows and narrow F0 ranges, so the kernel's edges -- a lag count of 63 / 64 / 65, more lags than a
workgroup of 256 has lanes, an odd window, a span at the LDS limit, the shortest signals -- are reached within a few dozen frames.
Every decision of a case (each d' against the threshold, each step down the dip, each parabola's sign, each gross comparison) is
decided by at least MARGIN relative, in float64 and in np.longdouble: that is what lets the GPU test compare voicing and lags exactly.
(A comparison of two exact zeros counts as decided -- ``yin_frame`` says why.)
"""
import functools
import os

import numpy as np

import audio_cases as C

MARGIN = 1e-9
FMIN, FMAX, THRESHOLD = 50.0, 500.0, 0.1        # the Python defaults
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = C.Case("tiny", 33, 64, 16, 16, 4)        # synthetic.tiny_hp()'s Sound section: n_fft 64, hop 16, 16 kHz
SHIPPED = C.Case("shipped", 513, 1024, 256, 80, 4)


def _frozen(a):
    a = np.array(a, order="C")
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ the tracker, restated
def lag_range(sr, fmin, fmax):
    """(tau_min, tau_max) = (floor(sr / fmax), ceil(sr / fmin)) in double, of the float32 values the C ABI carries."""
    return int(np.floor(float(sr) / float(np.float32(fmax)))), int(np.ceil(float(sr) / float(np.float32(fmin))))


def window_of(sr, window):
    return int(window) if window else int(np.floor(0.025 * sr + 0.5))


def frame_count(n, n_fft, hop, cap=None):
    nfr = 1 + n // hop if n > n_fft // 2 else 0
    return nfr if cap is None else min(nfr, cap)


def yin_frame(x, W, tau_min, tau_max, threshold, sr):
    """Steps 1-4 on one frame's W + tau_max samples ``x`` (float64 or longdouble; the arithmetic is x's).  Returns (f0, aperiodicity,
    lag -- 0 for unvoiced --, offset, margin): ``margin`` is the smallest relative distance by which a decision of this frame fell."""
    dt = x.dtype.type
    taus = np.arange(tau_max + 1)
    diff = x[:W, None] - x[np.arange(W)[:, None] + taus[None, :]]
    d = np.add.accumulate(diff * diff, axis=0)[-1]                      # one accumulator per lag, ascending j
    total = np.add.accumulate(d[1:])                                    # ascending k
    dp = np.ones(tau_max + 1, x.dtype)
    nz = total > 0
    dp[1:][nz] = d[1:][nz] * taus[1:][nz].astype(x.dtype) / total[nz]
    thr = dt(threshold)
    # A d or d' that is exactly 0 is so in any arithmetic (every term of its sum is the exact difference of two equal samples), so a
    # comparison of two exact zeros -- a burst that has left a zero-padded span -- falls the same way everywhere: it is decided.
    rel = lambda a, b: float(abs(a - b) / max(abs(a), abs(b))) if a != b else 1.0 if a == 0 else 0.0
    below = np.nonzero(dp[tau_min:tau_max] < thr)[0]
    if below.size == 0:
        margin = min((rel(v, thr) for v in dp[tau_min:tau_max]), default=1.0)
        return 0.0, float(dp[tau_min:tau_max + 1].min()), 0, 0.0, margin
    tau = tau_min + int(below[0])
    margin = min(rel(v, thr) for v in dp[tau_min:tau + 1])
    while tau + 1 < tau_max:
        margin = min(margin, rel(dp[tau + 1], dp[tau]))
        if not dp[tau + 1] < dp[tau]:
            break
        tau += 1
    a, b, c = d[tau - 1], d[tau], d[tau + 1]
    den = a - dt(2) * b + c
    margin = min(margin, float(abs(den) / (a + c)) if a + c > 0 else 1.0 if b == 0 else 0.0)
    off = (a - c) / (dt(2) * den) if den > 0 else dt(0)
    return float(dt(sr) / (dt(tau) + off)), float(dp[tau]), tau, float(off), margin


def pitch_reference(wav, case, top_db=None, fmin=FMIN, fmax=FMAX, threshold=THRESHOLD, window=0, cap=None, dtype=np.float64):
    """gsttaco_pitch of one row under ``case``'s Sound section -> dict(frames, f0, aperiodicity -- float64, NOT yet rounded to
    float32 --, lag, offset, margin [frames], start, n).  The trim (``top_db`` not None) is the oracle's, decided in float64."""
    wav = np.asarray(wav, np.float32)
    start, n = (0, wav.shape[0]) if top_db is None else C.trimmed(wav, top_db) if wav.shape[0] >= C.TRIM_FRAME // 2 + 1 else (0, 0)
    tau_min, tau_max = lag_range(case.sr, fmin, fmax)
    W = window_of(case.sr, window)
    L = W + tau_max
    nfr = frame_count(n, case.n_fft, case.hop, cap)
    thr = float(np.float32(threshold))
    y = np.concatenate([np.zeros(L, dtype), wav[start:start + n].astype(dtype), np.zeros(L + case.hop, dtype)])
    out = {k: np.zeros(nfr) for k in ("f0", "aperiodicity", "offset", "margin")}
    out["lag"] = np.zeros(nfr, np.int64)
    for t in range(nfr):
        u0 = t * case.hop - L // 2
        r = yin_frame(y[L + u0:L + u0 + L], W, tau_min, tau_max, thr, case.sr)
        out["f0"][t], out["aperiodicity"][t], out["lag"][t], out["offset"][t], out["margin"][t] = r
    out.update(frames=nfr, start=start, n=n, tau_min=tau_min, tau_max=tau_max, W=W)
    return out


# ------------------------------------------------------------------------------------------------ the error counts, restated
def pitch_errors_reference(fx, x_len, fy, y_len, path=None, path_len=None, gross=0.2, dtype=np.float64):
    """gsttaco_pitch_errors in plain loops -> (counts int32 [B, 6], sums float64 [B, 2], margin: the smallest relative distance of a
    gross comparison)."""
    fx, fy = np.asarray(fx, np.float32), np.asarray(fy, np.float32)
    B, Tx, Ty = fx.shape[0], fx.shape[1], fy.shape[1]
    dt = np.dtype(dtype).type
    g = dt(np.float32(gross))
    counts, sums, margin = np.zeros((B, 6), np.int32), np.zeros((B, 2), np.float64), 1.0
    for b in range(B):
        Lx = Tx if x_len is None else min(max(int(x_len[b]), 0), Tx)
        Ly = Ty if y_len is None else min(max(int(y_len[b]), 0), Ty)
        if path is None:
            cells = [(i, i) for i in range(min(Lx, Ly))]
        else:
            cells = [tuple(int(v) for v in path[b, s]) for s in range(min(max(int(path_len[b]), 0), path.shape[1]))]
        s1 = s2 = dt(0)
        for i, j in cells:
            if not (0 <= i < Lx and 0 <= j < Ly):
                continue
            x, y = dt(fx[b, i]), dt(fy[b, j])
            vx, vy = x > 0, y > 0
            counts[b] += (1, vx and vy, 0, vx != vy, vx, vy)
            if vx and vy:
                dev, lim = abs(x - y), g * y
                margin = min(margin, float(abs(dev - lim) / lim) if lim > 0 else 1.0)
                if dev > lim:
                    counts[b, 2] += 1
                else:
                    c = dt(1200) * np.log2(x / y)
                    s1, s2 = s1 + abs(c), s2 + c * c
        sums[b] = float(s1), float(s2)
    return counts, sums, margin


# ------------------------------------------------------------------------------------------------ signals
def sine(n, period, amp=0.3, phase=0.4, dtype=np.float32):
    return (amp * np.sin(2 * np.pi * np.arange(n) / float(period) + phase)).astype(dtype)


def harmonics(n, period, amps, dtype=np.float32):
    """sum_k amps[k - 1] sin(2 pi k t / period + k): a complex of fundamental period ``period``."""
    t = np.arange(n)
    return sum(a * np.sin(2 * np.pi * (k + 1) * t / float(period) + k + 1.0) for k, a in enumerate(amps)).astype(dtype)


def noise(n, seed, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


class PitchCase:
    """One call of gsttaco_pitch: ``rows`` (float32 signals) under ``sound`` (an audio_cases.Case) with the call's settings."""

    def __init__(self, name, sound, rows, top_db=None, fmin=FMIN, fmax=FMAX, threshold=THRESHOLD, window=0, expect=None):
        self.name, self.sound, self.top_db = name, sound, top_db
        self.rows = tuple(_frozen(np.asarray(r, np.float32)) for r in rows)
        self.fmin, self.fmax, self.threshold, self.window = fmin, fmax, threshold, window
        self.expect = expect or {}          # row -> the period (samples) its interior frames must find

    @property
    def settings(self):
        return dict(top_db=self.top_db, fmin=self.fmin, fmax=self.fmax, threshold=self.threshold, window=self.window)

    @property
    def span(self):
        return window_of(self.sound.sr, self.window) + lag_range(self.sound.sr, self.fmin, self.fmax)[1]


def _fastvox():
    g = np.load(os.path.join(GOLD, "audio_fv_all.npz"))
    return [g["pcm%d" % i].astype(np.float32) / 32768.0 for i in range(int(g["n"]))]


def _fmin_for(nlags):
    """An fmin whose tau_max + 1 is ``nlags`` at 16 kHz, half a lag away from either neighbour."""
    return 16000.0 / (nlags - 1.5)


H, HOP = TINY.n_fft // 2, TINY.hop
_NARROW = dict(fmin=_fmin_for(64), fmax=2000.0)          # lags 8 .. 63: what the small-window cases search


def _cases():
    cs = [
        # integer periods, W a multiple of P: d(P) = 0 and d(P - 1) = d(P + 1) in exact arithmetic
        PitchCase("sine_integer_periods", TINY, [sine(600, 20), sine(600, 32), sine(600, 40)], window=160, expect={0: 20, 1: 32, 2: 40},
                  **_NARROW),
        PitchCase("sine_between_periods", TINY, [sine(600, 20.3), sine(600, 33.7), sine(600, 47.21)], window=160,
                  expect={0: 20.3, 1: 33.7, 2: 47.21}, **_NARROW),
        # the fundamental missing (harmonics 2, 3, 4 of period 48); a second harmonic three times the fundamental: the first dip below
        # the threshold is the period's, not the stronger half period's, which never gets that low
        PitchCase("harmonic_complexes", TINY, [harmonics(700, 48, (0.0, 0.2, 0.2, 0.15)), harmonics(700, 44, (0.1, 0.3))], window=192,
                  expect={0: 48, 1: 44}, **_NARROW),
        PitchCase("noise_and_silence", TINY, [noise(500, 1), np.zeros(500, np.float32)], window=96, **_NARROW),
        PitchCase("voiced_between_noise", TINY, [np.concatenate([noise(320, 2, 0.05), sine(480, 25), noise(320, 3, 0.05)])], window=100,
                  **_NARROW),
    ]
    for nl in (63, 64, 65):
        cs.append(PitchCase("lags_%d" % nl, TINY, [sine(500, 29.4), harmonics(500, 37, (0.2, 0.1, 0.05))], window=96,
                            fmin=_fmin_for(nl), fmax=2000.0))
    cs += [
        # the default settings at the shipped Sound section: 321 lags (above 256 lanes, no multiple of 64), W = 400
        PitchCase("default_321_lags", SHIPPED, [harmonics(5000, 16000 / 118.0, (0.2, 0.15, 0.1, 0.05)), sine(4000, 16000 / 231.0)],
                  expect={0: 16000 / 118.0, 1: 16000 / 231.0}),
        PitchCase("odd_window", TINY, [sine(500, 26.6), noise(400, 4)], window=77, **_NARROW),
        # W + tau_max = 3071, one below the limit (few frames: the signal is short against the span)
        PitchCase("span_at_lds_limit", SHIPPED, [harmonics(4200, 16000 / 97.0, (0.2, 0.1, 0.1))], window=3071 - 320),
        # lengths n_fft/2 (no frame), n_fft/2 + 1, a multiple of the hop and one less
        PitchCase("length_edges", TINY, [sine(H, 21.5), sine(H + 1, 21.5), sine(10 * HOP, 21.5), sine(10 * HOP - 1, 21.5)], window=64, **_NARROW),
        PitchCase("ragged_batch", TINY, [sine(420, 24.8), np.zeros(20, np.float32), harmonics(333, 31, (0.2, 0.1)), noise(250, 5),
                                         sine(97, 18.2)], window=80, **_NARROW),
    ]
    # the audio_cases bursts: trimmed rows, 0-frame rows, the edge burst.  Lags 8 .. 101 hold the 69 samples after which the two tones
    # (700 Hz and 2.3 kHz) nearly repeat, so the rows have voiced frames whose position the trim moves
    wide = dict(fmin=16000.0 / 100.5, fmax=2000.0, window=64)
    for top_db in C.TOP_DBS:
        cs.append(PitchCase("trim_%d" % top_db, C.BY_NAME["short_window"], C.front_batch("short_window", top_db), top_db=top_db, **wide))
    cs.append(PitchCase("no_trim", C.BY_NAME["short_window"], C.front_batch("short_window", 60), top_db=None, **wide))
    cs.append(PitchCase("fastvox_defaults", SHIPPED, _fastvox(), top_db=15))
    return cs


CASES = {c.name: c for c in _cases()}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case_reference(name, dtype=np.float64):
    """Per row of the case: ``pitch_reference``'s dict (computed once, shared, frozen)."""
    c = CASES[name]
    out = []
    for row in c.rows:
        r = pitch_reference(row, c.sound, dtype=dtype, **c.settings)
        out.append({k: _frozen(v) if isinstance(v, np.ndarray) else v for k, v in r.items()})
    return tuple(out)


def interior_frames(ref, case):
    """The frames of a row whose whole span lies inside the signal (no zero reads)."""
    L = ref["W"] + ref["tau_max"]
    t = np.arange(ref["frames"])
    u0 = t * case.sound.hop - L // 2
    return t[(u0 >= 0) & (u0 + L <= ref["n"])]


# ------------------------------------------------------------------------------------------------ error-count cases
class ErrorCase:
    def __init__(self, name, fx, x_len, fy, y_len, path=None, path_len=None, gross=0.2, counts=None):
        self.name, self.gross = name, gross
        self.fx, self.fy = _frozen(np.asarray(fx, np.float32)), _frozen(np.asarray(fy, np.float32))
        i32 = lambda v: None if v is None else _frozen(np.asarray(v, np.int32))
        self.x_len, self.y_len, self.path, self.path_len = i32(x_len), i32(y_len), i32(path), i32(path_len)
        self.counts = None if counts is None else np.asarray(counts, np.int32)         # read off by inspection


def _error_cases():
    # row 0: (100,100) fine, (0,100) voicing, (130,100) gross, (0,0) nothing, (200,0) voicing, (119,100) fine
    # row 1: 120 against 100 with gross 0.2: |fx - fy| = 20 is NOT above float32(0.2) * 100 -- the comparison is strict; 120.01 is above
    fx = [[100, 0, 130, 0, 200, 119], [120, 120.01, 80, 79.99, 0, 0]]
    fy = [[100, 100, 100, 0, 0, 100], [100, 100, 100, 100, 0, 50]]
    by_hand = [[6, 3, 1, 2, 4, 4], [6, 4, 2, 1, 4, 5]]
    rng = np.random.default_rng(7)
    tx = np.where(rng.random((3, 40)) < 0.3, 0.0, rng.uniform(80, 300, (3, 40)))
    ty = np.where(rng.random((3, 50)) < 0.3, 0.0, rng.uniform(80, 300, (3, 50)))
    path = np.full((3, 89, 2), -1, np.int32)
    plen = np.zeros(3, np.int32)
    for b, (lx, ly) in enumerate(((40, 50), (17, 50), (40, 1))):       # a staircase from (0, 0) to (lx - 1, ly - 1)
        i = j = 0
        cells = [(0, 0)]
        while (i, j) != (lx - 1, ly - 1):
            step = rng.integers(0, 3)
            i, j = min(i + (step != 2), lx - 1), min(j + (step != 1), ly - 1)
            if (i, j) != cells[-1]:
                cells.append((i, j))
        path[b, :len(cells)] = cells
        plen[b] = len(cells)
    holes = np.array(path)
    holes[0, 5:9] = -1                                                  # -1 rows INSIDE the counted length, and cells beyond the lengths
    holes[1, 3] = (17, 2)
    holes[2, 2] = (3, 1)
    return [
        ErrorCase("by_inspection", fx, None, fy, None, counts=by_hand),
        ErrorCase("diagonal_unequal_lengths", tx, [40, 12, 0], ty[:, :45], [33, 45, 45]),
        ErrorCase("staircase_paths", tx, [40, 17, 40], ty, [50, 50, 1], path, plen),
        ErrorCase("paths_with_holes", tx, [40, 17, 40], ty, [50, 50, 1], holes, [89, int(plen[1]), int(plen[2])]),
        ErrorCase("zero_length_rows", tx, [0, 40, 5], ty, [50, 0, -3], path, plen, gross=0.35),
    ]


ERROR_CASES = {c.name: c for c in _error_cases()}
ERROR_NAMES = list(ERROR_CASES)


@functools.lru_cache(maxsize=None)
def error_reference(name, dtype=np.float64):
    c = ERROR_CASES[name]
    return pitch_errors_reference(c.fx, c.x_len, c.fy, c.y_len, c.path, c.path_len, c.gross, dtype)
