"""TEST INFRASTRUCTURE -- float64 NumPy restatements and shared cases of the validation-loss tests: what csrc/loss.hip computes (the
table in include/gsttaco.h), the reference's Train_Step reduction it must add up to (Model.py:210-241), and the linear spectrogram
target of gsttaco_feature_frontend (Audio.py:18-21).  tests/test_gpu_eval.py compares the device against these;
tests/test_eval_cases.py pins them on the CPU.
"""
import collections
import functools

import numpy as np
import scipy.fft

import audio_cases as C
from oracle import audio_np as A

FIELDS = ("pre_mel_l1", "mel_l1", "mel_l2", "stop_bce", "spec_l1", "spec_l2")
RTOL = 1e-9     # after the fp32 subtraction both sides are double and differ in summation order only: n * 2^-53 with n <= 1100 * 513
                # = 5.6e5 terms is 6e-11; 1e-9 is above that and 60 x below one fp32 rounding (6e-8), so an fp32 accumulator fails


def bce(x, z):
    """tf.nn.sigmoid_cross_entropy_with_logits in its stable form: max(x, 0) - x z + log(1 + exp(-|x|))."""
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    return np.maximum(x, 0.0) - x * z + np.log1p(np.exp(-np.abs(x)))


def bce_naive(x, z):
    """-z log(sigmoid(x)) - (1 - z) log(1 - sigmoid(x)): overflows / loses everything for large |x|."""
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    s = 1.0 / (1.0 + np.exp(-x))
    return -z * np.log(s) - (1.0 - z) * np.log(1.0 - s)


def _diff32(target, pred):
    """One fp32 subtraction per element, then double."""
    return (np.asarray(target, np.float32) - np.asarray(pred, np.float32)).astype(np.float64)


def losses(pre_mel, mel, stop, teacher, r, mel_lengths=None, spec=None, spec_target=None, spec_lengths=None):
    """float64 [B, 6] of gsttaco_losses: predictions [B, S*r, .] / [B, S], targets [B, Tq, .] with the go frame at index 0."""
    stop, teacher = np.asarray(stop), np.asarray(teacher)
    B, S = stop.shape
    T = teacher.shape[1] - 1
    assert T >= 1 and S * r >= T
    out = np.zeros((B, 6), np.float64)
    for b in range(B):
        L = T if mel_lengths is None else int(np.clip(mel_lengths[b], 0, T))
        d0 = _diff32(teacher[b, 1:1 + L], np.asarray(pre_mel)[b, :L])
        d1 = _diff32(teacher[b, 1:1 + L], np.asarray(mel)[b, :L])
        ch = teacher.shape[2]
        out[b, 0] = np.abs(d0).sum() / ch
        out[b, 1] = np.abs(d1).sum() / ch
        out[b, 2] = (d1 * d1).sum() / ch
        going = S if mel_lengths is None else max(0, -(-int(mel_lengths[b]) // r))
        out[b, 3] = bce(stop[b], (np.arange(S) < going)).sum()
        if spec is not None and spec_target is not None:
            Ls = T if spec_lengths is None else int(np.clip(spec_lengths[b], 0, T))
            d = _diff32(np.asarray(spec_target)[b, 1:1 + Ls], np.asarray(spec)[b, :Ls])
            out[b, 4] = np.abs(d).sum() / d.shape[-1] if Ls else 0.0
            out[b, 5] = (d * d).sum() / d.shape[-1] if Ls else 0.0
    return out


def sequence_mask(lengths, maxlen):
    return (np.arange(int(maxlen))[None, :] < np.asarray(lengths)[:, None]).astype(np.float64)


def train_step_loss(mels, mel_lengths, pre_mel_logits, mel_logits, stop_logits, r, spectrograms=None, spectrogram_lengths=None,
                    spectrogram_logits=None, use_l2=False):
    """Model.py:210-241 line by line on the padded arrays of a training batch: ``mels`` / ``spectrograms`` [B, T + 1, .] with the go
    frame, logits [B, T, .] and [B, T / r].  The differences are taken in the arrays' own dtype (float32, as TensorFlow takes them),
    everything after them in float64.  Returns {pre_mel, mel, stop, spectrogram, loss}."""
    f = np.float64
    T = mels.shape[1] - 1
    pre_Mel_Loss = np.mean(np.abs((mels[:, 1:] - pre_mel_logits).astype(f)), axis=-1)                        # :210
    mel_Loss = np.mean(np.abs((mels[:, 1:] - mel_logits).astype(f)), axis=-1)                                # :211
    if use_l2:
        mel_Loss = mel_Loss + np.mean(np.power((mels[:, 1:] - mel_logits).astype(f), 2), axis=-1)             # :214
    pre_Mel_Loss = pre_Mel_Loss * sequence_mask(mel_lengths, mel_Loss.shape[-1])                              # :217-221
    mel_Loss = mel_Loss * sequence_mask(mel_lengths, mel_Loss.shape[-1])                                      # :222-226
    labels = sequence_mask(np.ceil(np.asarray(mel_lengths) / r), np.ceil(mel_Loss.shape[-1] / r))             # :228-232
    stop_Loss = bce(stop_logits, labels)                                                                      # :227-234
    assert stop_Loss.shape == np.asarray(stop_logits).shape and T == mel_Loss.shape[-1]
    out = {"pre_mel": float(np.mean(pre_Mel_Loss)), "mel": float(np.mean(mel_Loss)), "stop": float(np.mean(stop_Loss)), "spectrogram": 0.0}
    if spectrograms is not None:
        spectrogram_Loss = np.mean(np.abs((spectrograms[:, 1:] - spectrogram_logits).astype(f)), axis=-1)    # :212
        if use_l2:
            spectrogram_Loss = spectrogram_Loss + np.mean(np.power((spectrograms[:, 1:] - spectrogram_logits).astype(f), 2), axis=-1)   # :215
        spectrogram_Loss = spectrogram_Loss * sequence_mask(spectrogram_lengths, spectrogram_Loss.shape[-1])  # :235-239
        out["spectrogram"] = float(np.mean(spectrogram_Loss))
    out["loss"] = out["pre_mel"] + out["mel"] + out["stop"] + out["spectrogram"]                              # :241
    return out


# ---------------------------------------------------------------------------------------------------- loss shapes
# The smallest shapes at which the loss kernel can go wrong.  T = Tq - 1; lengths None = the kernel's NULL; spec 0 = no spectrograms.
Shape = collections.namedtuple("Shape", "B T r mel spec lengths spec_lengths")
SHAPES = {
    "odd_channels": Shape(3, 7, 1, 80, 513, (7, 1, 4), (5, 7, 0)),         # 80 and 513 are not multiples of 64
    "label_edges": Shape(3, 9, 3, 80, 513, (9, 7, 1), (9, 7, 1)),          # ceil(len / r) = 3, 3, 1
    "trailing_frame": Shape(2, 8, 3, 16, 33, (8, 5), (8, 8)),              # S * r = 9 > T: the trailing prediction frame is never read
    "empty_row": Shape(2, 6, 2, 80, 0, (0, 6), None),                      # an all-zero row, its stop labels all 0; spectrogram NULL
    "long": Shape(1, 1100, 1, 80, 513, None, None),                        # more frames than threads
}
BIG_LOGITS = "label_edges"          # this row carries stop logits of +-100, where the naive bce overflows


def n_steps(shape):
    return -(-shape.T // shape.r)


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """Seeded fp32 tensors of a shape: dict(pre_mel, mel, stop, teacher, spec, spec_target, mel_lengths, spec_lengths).  The prediction
    frames t >= T (S * r > T) hold NaN: a kernel that read them would show it."""
    sh = SHAPES[name]
    rng = np.random.default_rng(1000 + sorted(SHAPES).index(name))
    S = n_steps(sh)

    def pred(ch):
        a = rng.normal(0.0, 1.5, (sh.B, S * sh.r, ch)).astype(np.float32)
        a[:, sh.T:] = np.nan
        return _frozen(a)

    def target(ch):
        return _frozen(np.clip(rng.normal(0.0, 1.5, (sh.B, sh.T + 1, ch)), -4.0, 4.0).astype(np.float32))

    stop = rng.normal(0.0, 3.0, (sh.B, S)).astype(np.float32)
    if name == BIG_LOGITS:
        stop[0, 0], stop[0, 2], stop[1, 1], stop[2, 0] = 100.0, -100.0, -100.0, 100.0       # both signs under both labels
    lens = None if sh.lengths is None else _frozen(np.array(sh.lengths, np.int32))
    slens = None if sh.spec_lengths is None else _frozen(np.array(sh.spec_lengths, np.int32))
    return dict(pre_mel=pred(sh.mel), mel=pred(sh.mel), stop=_frozen(stop), teacher=target(sh.mel),
                spec=pred(sh.spec) if sh.spec else None, spec_target=target(sh.spec) if sh.spec else None,
                mel_lengths=lens, spec_lengths=slens)


@functools.lru_cache(maxsize=None)
def loss_reference(name):
    c = loss_case(name)
    return _frozen(losses(c["pre_mel"], c["mel"], c["stop"], c["teacher"], SHAPES[name].r, c["mel_lengths"], c["spec"], c["spec_target"],
                          c["spec_lengths"]))


def _frozen(a):
    a = np.array(a, order="C")
    a.setflags(write=False)
    return a


def evaluation_layout(mel_List, spec_List, r):
    """Restatement of Feeder.py:103-143 for the mels and spectrograms of a training batch: zero-pad each to its own longest, prepend
    the zero go frame, pad both to the longer of the two rounded up to r, append one more frame."""
    def stack(items):
        n = max(m.shape[0] for m in items)
        out = np.zeros((len(items), n, items[0].shape[1]), np.float32)
        for i, m in enumerate(items):
            out[i, :m.shape[0]] = m
        return np.hstack([np.zeros((len(items), 1, items[0].shape[1]), np.float32), out])
    mels, specs = stack(mel_List), stack(spec_List)
    padded = np.maximum(mels.shape[1], specs.shape[1])
    padded = int(np.ceil(padded / r) * r)
    mels = np.hstack([mels, np.zeros((mels.shape[0], padded - mels.shape[1] + 1, mels.shape[2]), np.float32)])
    specs = np.hstack([specs, np.zeros((specs.shape[0], padded - specs.shape[1] + 1, specs.shape[2]), np.float32)])
    return mels, specs


# ---------------------------------------------------------------------------------------------------- the spectrogram target
def _normalise(S, case):
    return A.normalize(S) if case.max_abs is None else A.symmetric_normalize(S, max_abs_value=case.max_abs)


@functools.lru_cache(maxsize=None)
def spectrogram_reference(name, top_db):
    """Per wav of audio_cases.front_batch: the float64 linear spectrogram [frames, Spectrogram_Dim] of the signal Mel_Generate
    transforms (Pattern_Generator.py:39-60 up to the transform, then Audio.spectrogram, Audio.py:18-21), or None for a row the
    reference cannot transform."""
    case = C.BY_NAME[name]
    out = []
    for wav in C.front_batch(name, top_db):
        if C.expected_frames(case, wav, top_db) == 0:
            out.append(None)
            continue
        sig = A.preemphasis(np.asarray(wav))
        start, end = A.trim_bounds(sig, top_db, C.TRIM_FRAME, C.TRIM_HOP)
        sig = A.inv_preemphasis(sig[start:end] * 0.99)
        # (the oracle's stft rounds to complex64 as librosa's does; the dB and the normalisation of those magnitudes are float64 here)
        S = A.amp_to_db(A.magnitude(sig, case.n_fft, case.hop, case.win).astype(np.float64)) - 20
        out.append(_frozen(np.transpose(_normalise(S, case))))
        assert out[-1].shape == (C.expected_frames(case, wav, top_db), case.nb) and out[-1].dtype == np.float64
    return tuple(out)


def spectrogram_float32(case, wav, top_db):
    """The spectrogram as gt_stft_mel_kernel computes it, after audio_cases.mel_float32: float32 gather, window and real FFT, float32
    dB and normalisation, the trim decision in float64."""
    f = np.float32
    wav = np.asarray(wav, f)
    start, tlen = C.trimmed(wav, top_db)
    H = case.n_fft // 2
    prev = np.concatenate([[f(0)], wav[:-1]])
    x = ((wav - f(0.97) * prev) * f(0.99))[start:start + tlen]
    frames = A.frame(np.pad(x, H, mode="reflect"), case.n_fft, case.hop)
    mag = np.abs(scipy.fft.rfft(frames * C.padded_window(case, f)[:, None], axis=0))
    assert mag.dtype == f
    S = f(20) * np.log10(np.maximum(f(1e-5), mag)) - f(20)
    if case.max_abs is None:
        S = np.clip((S + f(100)) / f(100), f(0), f(1))
    else:
        m = f(case.max_abs)
        S = np.clip(f(2) * m * ((S + f(100)) / f(100)) - m, -m, m)
    assert S.dtype == f
    return S.T
