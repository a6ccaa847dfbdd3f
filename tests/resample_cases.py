"""Test infrastructure of the device resampler (gsttaco_resample, csrc/resample.hip): a float64 restatement of resampy's 'kaiser_best'
loop and the case table.

``restate`` follows ``oracle/audio_np.py::resample_kaiser_best`` tap for tap -- same table, same n / frac / offset / eta per wing, same
clipping of the tap counts -- but keeps everything in float64 and sums in the kernel's one fixed order: left wing tap 0 upward, then
right wing tap 0 upward.  Per output sample it returns the sum ``y64``, ``A = sum |w x|`` and the tap count ``N``, from which the tests
derive their bounds.

The time register.  resampy accumulates ``time += 1 / ratio`` in float64, once per output sample (``time="accumulated"``: numpy's
cumsum adds sequentially).  Because the table step is truncated (371 where scale * 512 is 371.52) the interpolation is discontinuous
where the register crosses an integer, and there the accumulated register often lies one rounding below the integer: a restatement
under the exact rational time t * sr_in / sr_out (``time="rational"``) lands 1e-4 away at such samples.  CASES 1 to 3 hold such samples
(tests/test_resample_cases.py asserts it), so a kernel that computes its time any other way fails them.

The GPU bound (``gpu_bound``), derived and not measured:  |y - y64| <= 2^-24 |y64| + N 2^-44 max|x|.  The first term is the one
rounding to float32.  The kernel accumulates in double: N additions and products of relative error 2^-53 each on partial sums of at
most A give N 2^-52 A, and A is at most a few times max|x| (the filter's absolute sum); 2^8 of room on top covers the library's own
window table (a power series for I0, a last-bit matter against scipy's) and its libm.
"""
import os

import numpy as np

from gst_tacotron_amd import audio

GOLDEN_LJ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_lj_excerpt.npz")
BITS = 512
SEED = 20250


def register(n_out, sr_in, sr_out, time="accumulated"):
    """(n, d): the integer part of the time register of outputs 0 .. n_out-1 and its fractional part as float64."""
    ratio = float(sr_out) / float(sr_in)
    if time == "accumulated":
        reg = np.concatenate([[0.0], np.cumsum(np.full(max(n_out - 1, 0), 1.0 / ratio))])[:n_out]      # sequential additions
        n = reg.astype(np.int64)
        return n, reg - n
    assert time == "rational"
    num = np.arange(n_out, dtype=np.int64) * int(sr_in)
    return num // int(sr_out), (num % int(sr_out)).astype(np.float64) / float(sr_out)


def restate(x, sr_in, sr_out, time="accumulated"):
    """-> (y64 [n_out], A [n_out], N [n_out], n_fix).  float64 throughout; see the module docstring."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n_orig = x64.shape[0]
    ratio = float(sr_out) / float(sr_in)
    n_out, n_fix = int(n_orig * ratio), int(np.ceil(n_orig * ratio))
    win = audio._kaiser_best() * (ratio if ratio < 1 else 1.0)
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    step = int(scale * BITS)
    nwin = win.shape[0]
    n, d = register(n_out, sr_in, sr_out, time)
    y, A, N = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, dtype=np.int64)
    if n_out == 0:
        return y, A, N, n_fix
    frac = scale * d
    for wing in (0, 1):
        if wing:
            frac = scale - frac
        index_frac = frac * BITS
        offset = index_frac.astype(np.int64)
        eta = index_frac - offset
        count = np.minimum((n + 1) if wing == 0 else (n_orig - n - 1), (nwin - offset) // step)
        for i in range(int(count.max()) if count.size else 0):
            ok = i < count
            idx = np.where(ok, offset + i * step, 0)
            src = np.clip((n - i) if wing == 0 else (n + i + 1), 0, n_orig - 1)
            term = (win[idx] + eta * delta[idx]) * x64[src]
            y = np.where(ok, y + term, y)
            A = np.where(ok, A + np.abs(term), A)
        N += np.maximum(count, 0)
    return y, A, N, n_fix


def reference(x, sr_in, sr_out, time="accumulated"):
    """``restate``, except at the target rate: nothing is resampled there (librosa.core.load, audio.load_wav), the row is its samples."""
    if sr_in != sr_out:
        return restate(x, sr_in, sr_out, time)
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    return x64, np.abs(x64), np.ones(x64.shape[0], dtype=np.int64), x64.shape[0]


def gpu_bound(y64, N, x):
    peak = float(np.abs(np.asarray(x, dtype=np.float64)).max()) if np.size(x) else 0.0
    return 2.0 ** -24 * np.abs(y64) + N * 2.0 ** -44 * peak


class Case:
    def __init__(self, number, sr_in, sr_out, n, what, x=None):
        self.number, self.sr_in, self.sr_out, self.n, self.what = number, sr_in, sr_out, n, what
        self.name = "%02d_%d_to_%d_n%d" % (number, sr_in, sr_out, n)
        self._x, self._ref = x, {}

    @property
    def x(self):
        """White noise of amplitude 0.5 from a fixed seed (its own per case), unless the case brought its samples."""
        if self._x is None:
            self._x = np.random.default_rng(SEED + self.number).uniform(-0.5, 0.5, self.n).astype(np.float32)
        return self._x

    def ref(self, time="accumulated"):
        """The restatement, computed once per process and shared by the tests that need it."""
        if time not in self._ref:
            self._ref[time] = reference(self.x, self.sr_in, self.sr_out, time)
        return self._ref[time]

    def padded(self):
        """y64 fix_length-ed to n_fix as float32: what the product returns."""
        y64, _, _, n_fix = self.ref()
        out = np.zeros(n_fix, dtype=np.float32)
        out[:y64.shape[0]] = y64.astype(np.float32)
        return out


def _lj():
    g = np.load(GOLDEN_LJ)
    assert int(g["sample_rate"]) == 22050 and int(g["target_rate"]) == 16000
    return g["pcm"].astype(np.float32) / 32768.0


CASES = [
    Case(1, 44100, 16000, 2001, "register case: step 185 of 185.76"),
    Case(2, 22050, 16000, 1000, "register case: step 371 of 371.52"),
    Case(3, 48000, 22050, 700, "register case: step 235 of 235.2"),
    Case(4, 48000, 16000, 1500, "an exact register (1 / ratio = 3) and the most taps per wing"),
    Case(5, 8000, 16000, 257, "up-sampling by 2: step 512, the table is not gained"),
    Case(6, 16000, 24000, 300, "up-sampling by 1.5"),
    Case(7, 11025, 16000, 600, "up-sampling by an awkward ratio"),
    Case(8, 16001, 16000, 400, "a ratio just below 1: step 511"),
    Case(9, 44100, 16000, 70, "shorter than one filter wing: both wings are clipped at every output"),
    Case(10, 22050, 16000, 2, "n_out 1, n_fix 2"),
    Case(11, 48000, 16000, 1, "n_out 0, n_fix 1: one zero sample"),
    Case(12, 16000, 16000, 333, "the pass-through"),
    Case(13, 22050, 16000, 33075, "the LJ excerpt", x=_lj()),
]
NAMES = [c.name for c in CASES]
BY_NUMBER = {c.number: c for c in CASES}
REGISTER_CASES = (1, 2, 3)
