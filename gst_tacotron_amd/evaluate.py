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
