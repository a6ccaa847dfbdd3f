"""Host side of ``GST_Tacotron.Evaluate``: how the per-utterance loss sums of ``gsttaco_losses`` become the numbers the reference's
``Train_Step`` reports (Model.py:210-241).  Plain NumPy on host values -- no device, no torch -- so that it can be driven without a GPU.

The columns (``LOSS_FIELDS``) are those of ``gsttaco_losses`` (include/gsttaco.h): per utterance SUMS over the frames below its length
of the per-frame channel means, and the sum of the stop token's cross entropy over all steps.
"""
import numpy as np

LOSS_FIELDS = ("pre_mel_l1", "mel_l1", "mel_l2", "stop_bce", "spec_l1", "spec_l2")


def use_l2_of(hp):
    """``Train.Use_L2_Loss`` of a hyper-parameter dict; False when the section or the key is absent (as in the shipped JSON)."""
    return bool((hp.get("Train") or {}).get("Use_L2_Loss", False))


def combine(sums, T, S, use_l2=False):
    """The five numbers of ``Train_Step`` from ``sums`` [B, 6] (``LOSS_FIELDS``), ``T`` = Tq - 1 padded target frames and ``S`` steps:
    {pre_mel, mel, stop, spectrogram, loss}, ``loss`` their sum (Model.py:241).

    Every frame term is sum_b / (B * T): the reference takes ``tf.reduce_mean`` over the whole padded [B, T] grid AFTER zeroing the
    frames beyond each length (Model.py:217-226, 235-241), so padding dilutes the mean -- a batch with one long and many short
    utterances reports a smaller loss than the same utterances evaluated in batches of similar lengths.  That quirk is the
    reference's and is kept; ``per_utterance_means`` is there for callers who want length-normalised numbers.  ``stop`` is
    sum_b / (B * S), unmasked (Model.py:227-234).  The L2 fields enter ``mel`` and ``spectrogram`` only with ``use_l2``
    (``Train.Use_L2_Loss``) and never ``pre_mel`` (Model.py:210-215)."""
    sums = np.asarray(sums, np.float64)
    if sums.ndim != 2 or sums.shape[1] != len(LOSS_FIELDS) or sums.shape[0] < 1:
        raise ValueError("sums must be [batch, {}]".format(len(LOSS_FIELDS)))
    if T < 1 or S < 1:
        raise ValueError("T and S must be at least 1")
    B = sums.shape[0]
    tot = sums.sum(axis=0)
    out = {"pre_mel": tot[0] / (B * T),
           "mel": (tot[1] + (tot[2] if use_l2 else 0.0)) / (B * T),
           "stop": tot[3] / (B * S),
           "spectrogram": (tot[4] + (tot[5] if use_l2 else 0.0)) / (B * T)}
    out["loss"] = out["pre_mel"] + out["mel"] + out["stop"] + out["spectrogram"]
    return {k: float(v) for k, v in out.items()}


def per_utterance_means(sums, lengths, spectrogram_lengths=None, steps=None):
    """``sums`` [B, 6] divided by each utterance's own length: the frame fields by ``lengths`` [B] (the spectrogram fields by
    ``spectrogram_lengths`` when given), ``stop_bce`` by ``steps`` (left a sum when None).  A length of 0 gives 0, not NaN."""
    sums = np.asarray(sums, np.float64)
    L = np.asarray(lengths, np.float64).reshape(-1)
    Ls = L if spectrogram_lengths is None else np.asarray(spectrogram_lengths, np.float64).reshape(-1)
    if sums.ndim != 2 or sums.shape[1] != len(LOSS_FIELDS) or L.shape != (sums.shape[0],) or Ls.shape != L.shape:
        raise ValueError("sums must be [batch, {}] and the lengths [batch]".format(len(LOSS_FIELDS)))
    out = sums.copy()
    for cols, n in (((0, 1, 2), L), ((4, 5), Ls)):
        for c in cols:
            out[:, c] = np.where(n > 0, sums[:, c] / np.maximum(n, 1.0), 0.0)
    if steps is not None:
        out[:, 3] = sums[:, 3] / float(steps)
    return out


# ---------------------------------------------------------------------------------------------------- the free-run metric (Evaluate_Free)
# Host side of ``GST_Tacotron.Evaluate_Free``: the constants of ``gsttaco_mel_dtw`` (include/gsttaco.h), stated once for the library's
# documentation and the test oracle, and how its per-utterance outputs become the reported numbers.
FREE_FIELDS = ("mcd", "cost", "path_len", "frames", "ref_frames", "duration_ratio", "stop_fired")


def dct_basis(n_ceps, mel_dim):
    """float64 [n_ceps, mel_dim]: rows k = 1 .. n_ceps of the orthonormal DCT-II over ``mel_dim`` channels,
    sqrt(2 / M) cos(pi k (2 m + 1) / (2 M)) -- c0 is dropped, so the rows are orthonormal (``basis @ basis.T`` = I) for n_ceps < mel_dim."""
    n_ceps, M = int(n_ceps), int(mel_dim)
    if not 1 <= n_ceps < M:
        raise ValueError("n_ceps must be in [1, mel_dim)")
    k = np.arange(1, n_ceps + 1, dtype=np.float64)[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / M) * np.cos(np.pi * k * (2.0 * m + 1.0) / (2.0 * M))


def mel_range(hp):
    """(low, high) of the normalised mel, what the reference's de-normalisation clips to (Audio.py:98-102): +-Sound.Max_Abs_Mel, or
    (0, 1) when that is 0 or absent.  The value is the float32 the context holds; without a complete Sound section
    ``capi.make_config`` leaves it 0, and so does this."""
    from .hparams import Dims
    d = Dims(hp)
    a = float(np.float32(d.max_abs_mel)) if d.audio else 0.0
    return (-a, a) if a > 0 else (0.0, 1.0)


def mcd_scale(hp):
    """What ``gsttaco_mel_dtw`` multiplies every feature by: g / sqrt(2) with g = dB per unit of the normalised mel = 100 / (2 Max_Abs_Mel)
    (100 for the [0, 1] normalisation).  With it the Euclidean distance of two frames' features is (10 / ln 10) sqrt(2 sum dc^2) on
    natural-log amplitude cepstra: the usual MCD in dB (derivation: include/gsttaco.h)."""
    lo, hi = mel_range(hp)
    return 100.0 / (hi - lo) / np.sqrt(2.0)


def combine_free(cost, path_len, frames, ref_frames, stop_step, steps):
    """float64 [B, len(FREE_FIELDS)] from ``gsttaco_mel_dtw``'s cost / path_len, the synthesis report's frames / stop_step
    (``REPORT_FIELDS``), the reference lengths and the step count S of the decode: mcd = cost / path_len (a ``path_len`` of 0 gives 0,
    not NaN), duration_ratio = frames / ref_frames (0 for ref_frames 0), stop_fired = 1 where stop_step < S."""
    cost = np.asarray(cost, np.float64).reshape(-1)
    cols = [np.asarray(v, np.float64).reshape(-1) for v in (path_len, frames, ref_frames, stop_step)]
    if any(c.shape != cost.shape for c in cols) or cost.shape[0] < 1:
        raise ValueError("cost, path_len, frames, ref_frames and stop_step must be [batch]")
    n, fr, ref, stop = cols
    out = np.zeros((cost.shape[0], len(FREE_FIELDS)), np.float64)
    out[:, 0] = np.where(n > 0, cost / np.maximum(n, 1.0), 0.0)
    out[:, 1], out[:, 2], out[:, 3], out[:, 4] = cost, n, fr, ref
    out[:, 5] = np.where(ref > 0, fr / np.maximum(ref, 1.0), 0.0)
    out[:, 6] = (stop < float(steps)).astype(np.float64)
    return out


def summarize_free(per_utterance):
    """{mcd: the mean over utterances of cost / path_len, mcd_frames: sum cost / sum path_len (0 for an empty sum)} of
    ``combine_free``'s result."""
    per = np.asarray(per_utterance, np.float64)
    n = per[:, 2].sum()
    return {"mcd": float(per[:, 0].mean()), "mcd_frames": float(per[:, 1].sum() / n) if n > 0 else 0.0}


# ---------------------------------------------------------------------------------------------------- the prosody metrics (Evaluate_Free(pitch=True))
# Host side of ``GST_Tacotron.Pitch_Errors``: how the per-utterance counts and sums of ``gsttaco_pitch_errors`` (include/gsttaco.h) become
# the triple the prosody-transfer literature reports beside MCD-DTW.
PITCH_COUNTS = ("pairs", "both_voiced", "gross", "voicing", "x_voiced", "y_voiced")
PITCH_FIELDS = ("gpe", "vde", "ffe", "f0_mae_cents", "f0_rmse_cents", "pairs", "both_voiced", "voiced_ratio")


def _ratio(num, den):
    """num / den element by element; a zero denominator gives 0, not NaN."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def combine_pitch(counts, sums):
    """float64 [B, len(PITCH_FIELDS)] from ``counts`` [B, 6] (``PITCH_COUNTS``) and ``sums`` [B, 2] (sum |c|, sum c^2 of the cents over
    the both-voiced, non-gross cells): gpe = gross / both_voiced (gross pitch error), vde = voicing / pairs (voicing decision error),
    ffe = (gross + voicing) / pairs (F0 frame error), f0_mae_cents = sum |c| / (both_voiced - gross), f0_rmse_cents =
    sqrt(sum c^2 / (both_voiced - gross)), voiced_ratio = x_voiced / y_voiced.  A zero denominator gives 0, not NaN."""
    counts, sums = np.asarray(counts, np.float64), np.asarray(sums, np.float64)
    if counts.ndim != 2 or counts.shape[1] != len(PITCH_COUNTS) or counts.shape[0] < 1 or sums.shape != (counts.shape[0], 2):
        raise ValueError("counts must be [batch, {}] and sums [batch, 2]".format(len(PITCH_COUNTS)))
    pairs, both, gross, voicing, xv, yv = (counts[:, k] for k in range(6))
    fine = both - gross
    out = np.zeros((counts.shape[0], len(PITCH_FIELDS)), np.float64)
    out[:, 0], out[:, 1], out[:, 2] = _ratio(gross, both), _ratio(voicing, pairs), _ratio(gross + voicing, pairs)
    out[:, 3], out[:, 4] = _ratio(sums[:, 0], fine), np.sqrt(_ratio(sums[:, 1], fine))
    out[:, 5], out[:, 6], out[:, 7] = pairs, both, _ratio(xv, yv)
    return out


def summarize_pitch(counts, sums):
    """{gpe, vde, ffe: the means over utterances of ``combine_pitch``'s columns; gpe_frames, vde_frames, ffe_frames: the same ratios of the
    counts summed over the batch (0 for an empty sum)} -- as ``summarize_free`` gives both the mean and the pooled figure."""
    per = combine_pitch(counts, sums)
    tot = np.asarray(counts, np.float64).sum(axis=0)
    out = {k: float(per[:, i].mean()) for i, k in enumerate(("gpe", "vde", "ffe"))}
    out["gpe_frames"] = float(_ratio(tot[2], tot[1]))
    out["vde_frames"] = float(_ratio(tot[3], tot[0]))
    out["ffe_frames"] = float(_ratio(tot[2] + tot[3], tot[0]))
    return out
