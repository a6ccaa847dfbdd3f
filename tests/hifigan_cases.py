"""The HiFi-GAN vocoder's float64 restatement and case table (tests/test_hifigan_cases.py admits the cases on the CPU,
tests/test_gpu_hifigan.py holds csrc/hifigan.hip to them).  ``hifigan_reference`` is written from the contract in include/gsttaco.h
(gsttaco_hifigan_config), row by row at each row's own length, in NumPy; ``dtype=np.float32`` runs the same chain in float32, whose
distance from the float64 run (``e32``) is the yardstick of the device's error: both are fp32 chains of one depth that differ in
summation order only."""
import functools
from dataclasses import dataclass

import numpy as np

from gst_tacotron_amd import hifigan
from vocoder_cases import _conv, _leaky, _pad16, _transposed, hifigan_plan_rule, tile_edge_frames, tile_form      # noqa: F401

MAX_ABS_MEL = 4.0
E32_MAX = 2.0 ** -14            # a case whose float32 run strays further from float64 is ill-conditioned: changed, not excused


# ---------------------------------------------------------------------------------------------------- the restatement
def hifigan_row(cfg, w, x):
    """One row alone: x [frames >= 1, mel_dim] -> [frames * hop]; the dtype is x's (the weights are cast to it)."""
    dt = x.dtype
    slope, out_slope = dt.type(cfg.slope), dt.type(cfg.out_slope)
    g = lambda name: np.asarray(w[name], dtype=dt)
    h = _conv(x, g("hifigan/in/kernel"), g("hifigan/in/bias"), 7, 1)
    for i, r in enumerate(cfg.rates):
        h = _transposed(_leaky(h, slope), g(f"hifigan/up{i}/kernel"), g(f"hifigan/up{i}/bias"), r)
        total = None
        for j, (k, dils) in enumerate(zip(cfg.kernels, cfg.dilations)):
            y = h
            for m, d in enumerate(dils):
                p = f"hifigan/up{i}/res{j}/unit{m}/"
                t = _conv(_leaky(y, slope), g(p + "conv1/kernel"), g(p + "conv1/bias"), k, d)
                if cfg.resblock == 1:
                    t = _conv(_leaky(t, slope), g(p + "conv2/kernel"), g(p + "conv2/bias"), k, 1)
                y = y + t
            total = y if total is None else total + y
        h = total * dt.type(1.0 / len(cfg.kernels))
    y = _conv(_leaky(h, out_slope), g("hifigan/out/kernel"), g("hifigan/out/bias"), 7, 1)
    return np.tanh(y[:, 0])


def hifigan_reference(cfg, weights, mel, frames=None, dtype=np.float64):
    """mel [B, T, mel_dim], frames [B] or None -> (wav [B, T * hop] of ``dtype``, lengths int32 [B]).  A row of 0 frames has length
    0; beyond a row's length the samples are zero; frames above T count as T."""
    mel = np.asarray(mel)
    B, T = mel.shape[:2]
    frames = np.full((B,), T) if frames is None else np.minimum(np.asarray(frames), T)
    wav = np.zeros((B, T * cfg.hop), dtype=dtype)
    lengths = np.zeros((B,), dtype=np.int32)
    for b in range(B):
        n = int(frames[b])
        if n < cfg.min_frames:
            continue
        wav[b, :n * cfg.hop] = hifigan_row(cfg, weights, mel[b, :n].astype(dtype))
        lengths[b] = n * cfg.hop
    return wav, lengths


# ---------------------------------------------------------------------------------------------------- the plan's constants
def plan_tiles(cfg):
    """What gsttaco_hifigan_plan reports as (kind, channels, taps, dilation, tile, form, rate) per launch: one launch per convolution;
    the N-tiles a wave item owns by padded channel count, and the time tile that gives four waves an item each, halved while the
    launch's LDS does not fit (vocoder_cases.hifigan_plan_rule)."""
    return [(s["kind"], s["channels"], s["taps"], s["dilation"], s["tile"], s["form"], s["rate"]) for s in hifigan_plan_rule(cfg)]


# ---------------------------------------------------------------------------------------------------- the cases
@dataclass
class Case:
    name: str
    cfg: hifigan.HiFiGANConfig
    frames: tuple
    seed: int
    hot: bool = False

    @property
    def T(self):
        return max(max(self.frames), 1)

    @functools.cached_property
    def weights(self):
        w = hifigan.synthetic_weights(self.cfg, seed=self.seed)
        if self.hot:
            # every hidden layer's bias pulled down, so most pre-activations are negative and the LeakyReLU's slope branch carries
            # the signal; the output conv scaled up until the tanh saturates on part of the waveform
            for name in w:
                if name.endswith("/bias") and name != "hifigan/out/bias":
                    w[name] = (w[name] - 0.75).astype(np.float32)
            w["hifigan/out/kernel"] = (w["hifigan/out/kernel"] * 6.0).astype(np.float32)
        return w

    @functools.cached_property
    def mel(self):
        rng = np.random.default_rng(1000 + self.seed)
        B, T, D = len(self.frames), self.T, self.cfg.mel_dim
        if self.hot:
            x = np.where(rng.random((B, T, D)) < 0.5, -MAX_ABS_MEL, MAX_ABS_MEL)
        else:
            x = np.clip(rng.normal(0.0, 1.5, (B, T, D)), -MAX_ABS_MEL, MAX_ABS_MEL)
        return x.astype(np.float32)         # (frames beyond a row's length hold values too: they must not be read)

    @property
    def frames_array(self):
        return np.asarray(self.frames, dtype=np.int32)


_C = hifigan.HiFiGANConfig
# k = 11 at d = 5 has a halo of 25 a side, and with the closing conv's 5 a unit reaches 30: at rates [2, 2] the first stage's rows
# are 24 .. 32 samples (lengths are even: 24 / 26 straddle 25; 28 / 30 / 32 are below, at and the next length above 30)
_HALO = _C(mel_dim=5, initial=8, rates=[2, 2], resblock=1, kernels=[11, 3], dilations=[[5], [1]])
_TILES = _C(mel_dim=80, initial=32)
CASES = {c.name: c for c in (
    Case("tiny", _C(mel_dim=5, initial=8, rates=[2, 2], resblock=1, kernels=[3, 5], dilations=[[4, 5], [3]]), (9, 1, 2, 0), 1),
    Case("odd_channels", _C(mel_dim=7, initial=12, rates=[4, 2], resblock=2, kernels=[3, 5, 11], dilations=[[1, 2], [3], [1, 5]]), (7, 5), 2),
    Case("one_kernel", _C(mel_dim=5, initial=8, rates=[2, 2], resblock=1, kernels=[3], dilations=[[1, 3]]), (6, 3), 3),
    Case("one_kernel_v3", _C(mel_dim=5, initial=8, rates=[2, 2], resblock=2, kernels=[5], dilations=[[2]]), (6, 1), 8),
    Case("halo", _HALO, (12, 13, 14, 15, 16), 4),
    Case("tiles", _TILES, tuple(tile_edge_frames(plan_tiles(_TILES))), 5),
    Case("v1", _C.v1(), (12, 7), 6),
    Case("v3", _C.v3(), (12, 7), 9),
    Case("hot", _C(mel_dim=8, initial=16, rates=[4, 2], resblock=1, kernels=[3, 5], dilations=[[1, 3], [2]]), (11, 6), 7, hot=True),
)}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float64"):
    """(wav, lengths) of a case, computed once and shared; callers leave it unchanged."""
    c = CASES[name]
    wav, lengths = hifigan_reference(c.cfg, c.weights, c.mel, c.frames_array, dtype=np.dtype(dtype).type)
    wav.setflags(write=False)
    lengths.setflags(write=False)
    return wav, lengths


@functools.lru_cache(maxsize=None)
def e32(name):
    """max |float32 run - float64 run| of the restatement over the case"""
    return float(np.abs(reference(name, "float32")[0].astype(np.float64) - reference(name)[0]).max())
