"""The NumPy pieces the vocoders' float64 restatements share (tests/melgan_cases.py, hifigan_cases.py, waveglow_cases.py) and the
plan's tile rule of csrc/vocoder_common.h.  Every function keeps the dtype of its input."""
import numpy as np


def _leaky(x, slope):
    return np.where(x > 0, x, x * slope)


def _conv(x, w, b, taps, dil):
    """x [L, cin], w [taps * cin, cout] -> [L, cout], taps odd: zero padding (taps - 1) / 2 * dil each side; bias, then taps ascending"""
    cin = w.shape[0] // taps
    L, p = x.shape[0], (taps - 1) // 2 * dil
    xp = np.pad(x, ((p, p), (0, 0)))
    y = np.tile(b[None, :], (L, 1))
    for k in range(taps):
        y = y + xp[k * dil:k * dil + L] @ w[k * cin:(k + 1) * cin]
    return y


def _reflect(x, p):
    return np.pad(x, ((p, p), (0, 0)), mode="reflect")


def _transposed(x, w, b, r):
    """x [L, cin], w [2r, cin, cout]: output o = i r - r/2 + k, cropped to [0, r L): two taps per sample, nothing beyond the ends"""
    L = x.shape[0]
    full = np.zeros(((L + 1) * r, w.shape[2]), dtype=x.dtype)
    for k in range(2 * r):
        full[k:k + (L - 1) * r + 1:r] += x @ w[k]
    return full[r // 2:r // 2 + r * L] + b[None, :]


def _pad16(c):
    return (c + 15) // 16 * 16


def tile_form(n_p):
    """(time tile, N-tiles a wave item owns) of a launch of n_p padded output channels: the form by channel count, and the tile that
    gives four waves an item each"""
    ntiles = n_p // 16
    nt = 4 if ntiles % 4 == 0 and ntiles >= 16 else (2 if ntiles % 2 == 0 else 1)
    ngroups = ntiles // nt
    return 64 * (1 if ngroups >= 4 else 2 if ngroups >= 2 else 4), nt


def tile_edge_frames(tiles, min_frames=1):
    """One, zero and one more frame around the first and second multiple of each launch's time tile that a whole frame count
    reaches.  ``tiles``: rows that end in (tile, form, rate).  Frame counts below ``min_frames`` stay in (MelGAN's short rows must
    come out empty)."""
    frames = set()
    for *_, tile, _, rate in tiles:
        for m in (1, 2):
            if (m * tile) % rate == 0:
                f = m * tile // rate
                frames.update(v for v in (f - 1, f, f + 1) if v >= 1)
    return sorted(frames)
