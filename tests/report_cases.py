"""TEST INFRASTRUCTURE -- NumPy restatements of what csrc/report.hip computes: the synthesis report of gsttaco_utterance_report (the
table in include/gsttaco.h, float64) and the per-utterance-seeded randomness of gsttaco_fill_randomness, built row by row from
oracle/rng_np.py's batch-of-one tensors.  The GPU tests compare against these; tests/test_report_cases.py pins them."""
import numpy as np

from oracle import rng_np

FIELDS = ("stop_step", "frames", "end_gap", "max_jump", "back_steps", "max_stall", "visited", "nonfinite")


def report(stop, align, r, token_lengths=None, mel=None):
    """(report int32 [B, 8], focus float64 [B]) of stop [B, S], align [B, S, Tv], token_lengths [B] or None, mel [B, S*r, mel_dim] or
    None.  With non-finite values inside the counted region fields 2..6 and focus are whatever numpy.argmax / max make of them."""
    stop, align = np.asarray(stop), np.asarray(align)
    B, S, Tv = align.shape
    assert stop.shape == (B, S)
    out = np.zeros((B, 8), np.int32)
    focus = np.zeros(B, np.float64)
    for b in range(B):
        n = Tv if token_lengths is None else int(np.clip(token_lengths[b], 1, Tv))
        neg = np.flatnonzero(stop[b] < 0)                      # (a NaN is not below 0)
        first = int(neg[0]) if neg.size else S                 # Model.py:380
        E = min(S, max(1, first))
        frames = max(1, first) * r                             # Model.py:413
        win = align[b, :E, :n].astype(np.float64)
        a = np.argmax(win, axis=1)                             # (the lowest index on a tie)
        d = np.diff(a)
        run = best = 1
        for x in d:
            run = run + 1 if x == 0 else 1
            best = max(best, run)
        nonfinite = int((~np.isfinite(stop[b, :E])).sum()) + int((~np.isfinite(win)).sum())
        if mel is not None:
            nonfinite += int((~np.isfinite(np.asarray(mel)[b, :frames])).sum())
        out[b] = (first, frames, (n - 1) - int(a.max()), max(0, int(d.max())) if d.size else 0, int((d < 0).sum()), best,
                  len(set(a.tolist())), nonfinite)
        focus[b] = win.max(axis=1).mean()
    return out, focus


def randomness(seeds, steps, Tv, prenet, rate):
    """(masks float32 [steps, 2, B, prenet], noise float64 [steps, B, Tv]): row b is the row of a batch of ONE under seed seeds[b]."""
    B = len(seeds)
    masks = np.empty((steps, 2, B, prenet), np.float32)
    noise = np.empty((steps, B, Tv), np.float64)
    for b, seed in enumerate(seeds):
        masks[:, :, b, :] = rng_np.masks(int(seed), steps, 1, prenet, prenet, rate).reshape(steps, 2, prenet)
        noise[:, b, :] = rng_np.noise(int(seed), steps, 1, Tv)[:, 0, :]
    return masks, noise


def one_hot_path(path, Tv, peak=0.9):
    """align [1, len(path), Tv]: a sharp alignment that sits at token path[s] at step s (the rest of the row shares 1 - peak)."""
    a = np.full((1, len(path), Tv), (1.0 - peak) / max(1, Tv - 1), np.float32)
    a[0, np.arange(len(path)), np.asarray(path)] = peak
    return a
