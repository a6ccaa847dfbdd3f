"""Sound sections, signals and shared float64 references of the audio-kernel tests (csrc/audio.hip): tests/test_gpu_audio.py runs
them on the GPU, tests/test_audio_cases.py checks on the CPU that they are well conditioned and can see what they are meant to see.

tests/test_audio.py runs the front end (wav -> mels_for_gst) and Griffin-Lim at the shipped Sound section and synthetic.tiny_hp()'s:
both have Frame_Length == n_fft, Frame_Shift == n_fft / 4 and Max_Abs_Mel 4.  The sections here leave each of those, one or two at
a time:

    short_window            a zero-padded, centred window (48 in 64) and its sum-square
    odd_window_hop12_unit   an odd window (51 in 64: left pad 6, right pad 7), a hop that does not divide n_fft, the [0, 1] normalisation
    half_overlap            hop = n_fft / 2: two frames cover a sample, the window sum-square dips to 0.5 of its peak
    nfft2048                1024 complex points in the LDS FFT: the first size at which a thread does two butterflies per stage

No case has Frame_Shift >= Frame_Length: there the window sum-square touches zero between frames, the oracle's own waveform peaks
near 100 and the comparison would measure librosa's `tiny` threshold, not the kernel.
"""
import copy
import functools

import numpy as np
import scipy.fft

from gst_tacotron_amd import hparams
from oracle import audio_np as A

MEL_TOL = 2e-3          # tests/test_audio.py's: float32 FFT / log10 against the float64 oracle, mel values in [-4, 4]
GL_TOL = 2e-3           # tests/test_audio.py::test_gpu_griffin_lim_matches_oracle's: relative to the oracle waveform's peak
GL_ITERS = (0, 2)
GL_POWER, GL_REF_DB = 1.2, 15.0         # not the defaults 1.5 / 20
GL_FRAMES = 11                          # frames of every Griffin-Lim spectrogram
TOP_DBS = (60, 15)
TRIM_FRAME, TRIM_HOP = 32, 16           # Pattern_Generator.py:45
SEED64 = 0x9E3779B97F4A7C15             # a seed with a non-zero high word


class Case:
    def __init__(self, name, spec_dim, frame_length, frame_shift, mel_dim, max_abs, sample_rate=16000, seed=0):
        self.name, self.seed = name, seed
        self.sound = {"Spectrogram_Dim": spec_dim, "Mel_Dim": mel_dim, "Frame_Length": frame_length, "Frame_Shift": frame_shift,
                      "Sample_Rate": sample_rate, "Max_Abs_Mel": max_abs}
        self.n_fft, self.win, self.hop, self.mel, self.max_abs, self.sr = 2 * (spec_dim - 1), frame_length, frame_shift, mel_dim, max_abs, sample_rate
        self.nb = spec_dim
        assert self.hop < self.win <= self.n_fft

    @property
    def mel_tol(self):
        """MEL_TOL is for values spanning 8 units per 100 dB; the [0, 1] normalisation spans 1."""
        return MEL_TOL if self.max_abs is not None else MEL_TOL / 8

    @property
    def mel_floor(self):
        return -float(self.max_abs) if self.max_abs is not None else 0.0

    @property
    def k0(self):
        """The largest frame count Griffin-Lim cannot invert: Frame_Shift * (k0 - 1) <= n_fft / 2 (librosa.stft's reflect padding)."""
        return (self.n_fft // 2) // self.hop + 1

    def hp(self):
        hp = copy.deepcopy(hparams.load_hp())
        hp["Sound"].update(self.sound)
        return hp


CASES = [
    Case("short_window", 33, 48, 16, 16, 4, seed=11),
    Case("odd_window_hop12_unit", 33, 51, 12, 16, None, seed=12),
    Case("half_overlap", 65, 128, 64, 16, 4, seed=13),
    Case("nfft2048", 1025, 1200, 300, 80, 4, sample_rate=24000, seed=14),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
PADDED_WINDOW = ["short_window", "odd_window_hop12_unit"]       # the 64-point cases with Frame_Length < n_fft


def _frozen(a):
    a = np.array(a, order="C")
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ signals
def signal(case, n, seed, edges=True):
    """Two tones plus white noise at 0.01, float32.  With ``edges``: the first and last 15 % scaled by 1e-4 (cut by the trim at
    top_db 60 and 15) and the next 10 % on either side by 0.05 (-26 dB: cut at 15, kept at 60)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(case.sr)
    f1, f2 = 0.044 * case.sr, 0.145 * case.sr                   # 700 Hz and 2.3 kHz at 16 kHz
    y = 0.08 * np.sin(2 * np.pi * f1 * t + 0.3) + 0.03 * np.sin(2 * np.pi * f2 * t + 1.1) + 0.01 * rng.standard_normal(n)
    if edges:
        e, s = int(0.15 * n), int(0.25 * n)
        env = np.ones(n)
        env[:s] = env[n - s:] = 0.05
        env[:e] = env[n - e:] = 1e-4
        y = y * env
    return _frozen(y.astype(np.float32))


def trimmed(wav, top_db):
    """(start, length) the reference's trim keeps (Pattern_Generator.py:45), decided in float64 like the reference."""
    s, e = A.trim_bounds(A.preemphasis(np.asarray(wav)), top_db, TRIM_FRAME, TRIM_HOP)
    return s, e - s


@functools.lru_cache(maxsize=None)
def edge_wav(name, top_db):
    """A burst at the end of a silent buffer whose trimmed length lands in (n_fft/2, n_fft/2 + 16]: the shortest signals
    librosa.stft accepts, where the single reflection of the padding is at its limit."""
    case = BY_NAME[name]
    H = case.n_fft // 2
    rng = np.random.default_rng(case.seed + 500)
    burst = 0.1 * rng.standard_normal(H + 3 * TRIM_HOP)
    for n in range(H + 1, H + 3 * TRIM_HOP):
        wav = np.zeros(3 * H + n, np.float32)
        wav[-n:] = burst[:n]
        if H < trimmed(wav, top_db)[1] <= H + TRIM_HOP:
            return _frozen(wav)
    raise AssertionError("no burst length lands the trimmed length in (n_fft/2, n_fft/2 + 16]")


@functools.lru_cache(maxsize=None)
def front_batch(name, top_db):
    """The five wavs of the front-end batch: full length (6 n_fft), shorter, 300 zeros, 17 samples, the edge burst."""
    case = BY_NAME[name]
    return (signal(case, 6 * case.n_fft, case.seed), signal(case, 7 * case.n_fft // 2 + 5, case.seed + 100),
            _frozen(np.zeros(300, np.float32)), signal(case, 17, case.seed + 200, edges=False), edge_wav(name, top_db))


def expected_frames(case, wav, top_db):
    """mel_lengths of a wav: 1 + trimmed // hop, or 0 where the reference raises (trimmed length <= n_fft / 2)."""
    tlen = trimmed(wav, top_db)[1]
    return 1 + tlen // case.hop if tlen > case.n_fft // 2 else 0


@functools.lru_cache(maxsize=None)
def front_reference(name, top_db):
    """Per wav of front_batch: the oracle's float32 mels [frames, Mel_Dim], or None for a row the reference cannot transform."""
    case = BY_NAME[name]
    out = []
    for wav in front_batch(name, top_db):
        if expected_frames(case, wav, top_db) == 0:
            out.append(None)
        else:
            out.append(_frozen(A.mel_generate(np.array(wav), case.sound, top_db)))
            assert out[-1].shape == (expected_frames(case, wav, top_db), case.mel)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ front end, restated in float32
def padded_window(case, dtype=np.float64, shift=0):
    """hann(Frame_Length) centred in n_fft (librosa.util.pad_center), optionally ``shift`` samples off centre."""
    lpad = (case.n_fft - case.win) // 2 + shift
    w = np.zeros(case.n_fft, dtype)
    w[lpad:lpad + case.win] = A.hann_periodic(case.win)
    return w


def mel_float32(case, wav, top_db, window_shift=0):
    """The front end as gt_stft_mel_kernel computes it -- float32 gather of 0.99 x the pre-emphasised trimmed signal, float32 window,
    float32 real FFT, float32 mel basis and dB -- with the trim decision in float64.  ``window_shift`` moves the window inside the
    padded frame: what a wrong left pad would do."""
    f = np.float32
    wav = np.asarray(wav, f)
    start, tlen = trimmed(wav, top_db)
    H = case.n_fft // 2
    prev = np.concatenate([[f(0)], wav[:-1]])
    x = ((wav - f(0.97) * prev) * f(0.99))[start:start + tlen]
    frames = A.frame(np.pad(x, H, mode="reflect"), case.n_fft, case.hop)
    w = padded_window(case, f, window_shift)
    mag = np.abs(scipy.fft.rfft(frames * w[:, None], axis=0))
    assert mag.dtype == f
    S = f(20) * np.log10(np.maximum(f(1e-5), A.mel_basis(case.sr, case.n_fft, case.mel) @ mag))
    if case.max_abs is None:
        S = np.clip((S + f(100)) / f(100), f(0), f(1))
    else:
        m = f(case.max_abs)
        S = np.clip(f(2) * m * ((S + f(100)) / f(100)) - m, -m, m)
    assert S.dtype == f
    return S.T


# ------------------------------------------------------------------------------------------------ Griffin-Lim inputs
@functools.lru_cache(maxsize=None)
def spectrogram(name, row):
    """Normalised linear spectrogram [GL_FRAMES, bins] (float32) of a two-tone signal under the case's section (Audio.spectrogram,
    Audio.py:18-21), as tests/test_audio.py::_realistic_spectrogram builds it."""
    case = BY_NAME[name]
    y = np.array(signal(case, case.hop * (GL_FRAMES - 1), case.seed + 300 + row, edges=False), np.float64)
    S = A.amp_to_db(A.magnitude(y, case.n_fft, case.hop, case.win)) - 20
    S = A.normalize(S) if case.max_abs is None else A.symmetric_normalize(S, max_abs_value=case.max_abs)
    assert S.shape == (case.nb, GL_FRAMES)
    return _frozen(np.transpose(S).astype(np.float32))


@functools.lru_cache(maxsize=None)
def gl_batch(name):
    """(spectrograms [5, T, bins], frames [T, 0, 1, k0, k0 + 1], initial phases [5, T, bins] in [0, 1)), float32 / int32."""
    case = BY_NAME[name]
    spec = np.stack([spectrogram(name, r) for r in range(5)])
    frames = np.array([GL_FRAMES, 0, 1, case.k0, case.k0 + 1], np.int32)
    assert case.k0 + 1 <= GL_FRAMES and case.hop * (case.k0 - 1) <= case.n_fft // 2 < case.hop * case.k0
    ph = np.random.default_rng(case.seed + 400).random(spec.shape).astype(np.float32)
    return _frozen(spec), _frozen(frames), _frozen(ph)


@functools.lru_cache(maxsize=None)
def gl_reference(name, row, frames, iters):
    """The oracle's waveform of the first ``frames`` frames of a row (float64), at GL_POWER / GL_REF_DB."""
    case = BY_NAME[name]
    spec, _, ph = gl_batch(name)
    y = A.inv_spectrogram(spec[row, :frames].T.astype(np.float64), case.sound, ref_level_db=GL_REF_DB, power=GL_POWER,
                          max_abs_value=case.max_abs, iters=iters, angles0=ph[row, :frames].T.astype(np.float64))
    assert y.shape == (case.hop * (frames - 1),)
    return _frozen(y)


# ------------------------------------------------------------------------------------------------ Griffin-Lim, restated in float32
def inv_spectrogram_float32(case, spec, phases, iters, wss_shift=None):
    """Audio.inv_spectrogram with every array in float32 and scipy.fft's float32 transforms (what the kernels' arithmetic is), the
    window sum-square accumulated like librosa's.  ``spec`` / ``phases``: [T, bins].  ``wss_shift``: None for librosa's sum-square
    (the squared window centred in n_fft like the window); an integer places the squared window that many samples off centre
    (-(n_fft - Frame_Length) // 2: the unpadded window's position, index 0)."""
    f = np.float32
    N, hop, T = case.n_fft, case.hop, spec.shape[0]
    spec = np.asarray(spec, f).T
    if case.max_abs is None:
        db = np.clip(spec, f(0), f(1)) * f(100) - f(100)
    else:
        m = f(case.max_abs)
        db = (np.clip(spec, -m, m) + m) / (f(2) * m) * f(100) - f(100)
    S = np.exp(f(GL_POWER) * f(0.11512925464970229) * (db + f(GL_REF_DB)))
    w = padded_window(case, f)
    wsq = padded_window(case, np.float64, 0 if wss_shift is None else wss_shift) ** 2
    n = N + hop * (T - 1)
    wss = np.zeros(n, f)
    for i in range(T):
        wss[i * hop:i * hop + N] += wsq

    def istft(D):
        fr = scipy.fft.irfft(D, n=N, axis=0) * w[:, None]
        assert fr.dtype == f
        y = np.zeros(n, f)
        for i in range(T):
            y[i * hop:i * hop + N] += fr[:, i]
        nz = wss > np.finfo(f).tiny
        y[nz] /= wss[nz]
        return y[N // 2:-(N // 2)]

    ang = (f(2 * np.pi) * np.asarray(phases, f).T)
    D = (S * (np.cos(ang) + 1j * np.sin(ang))).astype(np.complex64)
    y = istft(D)
    for _ in range(iters):
        X = scipy.fft.rfft(A.frame(np.pad(y, N // 2, mode="reflect"), N, hop) * w[:, None], axis=0)
        r = np.abs(X)
        unit = np.where(r > 0, X / np.where(r > 0, r, 1), 1).astype(np.complex64)
        y = istft(S * unit)
    return A.inv_preemphasis(y.astype(np.float64))
