"""The neural vocoder's float64 restatement and case table (tests/test_melgan_cases.py admits the cases on the CPU,
tests/test_gpu_melgan.py holds csrc/melgan.hip to them).  ``melgan_reference`` is written from the contract in include/gsttaco.h
(gsttaco_melgan_config), row by row at each row's own length, in NumPy; ``dtype=np.float32`` runs the same chain in float32, whose
distance from the float64 run (``e32``) is the yardstick of the device's error: both are fp32 chains of one depth that differ in
summation order only."""
import functools
from dataclasses import dataclass

import numpy as np

from gst_tacotron_amd import melgan
from vocoder_cases import _leaky, _pad16, _reflect, _transposed, melgan_plan_rule, tile_edge_frames, tile_form      # noqa: F401

MAX_ABS_MEL = 4.0
E32_MAX = 2.0 ** -14            # a case whose float32 run strays further from float64 is ill-conditioned: changed, not excused


# ---------------------------------------------------------------------------------------------------- the restatement
def _conv(x, w, b, taps, dil):
    """x [L + (taps - 1) dil, cin] (already padded: MelGAN reflects, so this is not vocoder_cases._conv, which pads with zeros),
    w [taps * cin, cout] -> [L, cout]"""
    cin = w.shape[0] // taps
    L = x.shape[0] - (taps - 1) * dil
    y = np.tile(b[None, :], (L, 1))
    for k in range(taps):
        y = y + x[k * dil:k * dil + L] @ w[k * cin:(k + 1) * cin]
    return y


def melgan_row(cfg, w, x):
    """One row alone: x [frames >= min_frames, mel_dim] -> [frames * hop]; the dtype is x's (the weights are cast to it)."""
    dt = x.dtype
    slope = dt.type(cfg.slope)
    g = lambda name: np.asarray(w[name], dtype=dt)
    h = _conv(_reflect(x, 3), g("melgan/in/kernel"), g("melgan/in/bias"), 7, 1)
    for i, r in enumerate(cfg.ratios):
        h = _transposed(_leaky(h, slope), g(f"melgan/up{i}/kernel"), g(f"melgan/up{i}/bias"), r)
        for j in range(cfg.n_res):
            p, d = f"melgan/up{i}/res{j}/", 3 ** j
            t = _conv(_reflect(_leaky(h, slope), d), g(p + "conv3/kernel"), g(p + "conv3/bias"), 3, d)
            t = _conv(_leaky(t, slope), g(p + "conv1/kernel"), g(p + "conv1/bias"), 1, 1)
            h = _conv(h, g(p + "shortcut/kernel"), g(p + "shortcut/bias"), 1, 1) + t
    y = _conv(_reflect(_leaky(h, slope), 3), g("melgan/out/kernel"), g("melgan/out/bias"), 7, 1)
    return np.tanh(y[:, 0])


def melgan_reference(cfg, weights, mel, frames=None, dtype=np.float64):
    """mel [B, T, mel_dim], frames [B] or None -> (wav [B, T * hop] of ``dtype``, lengths int32 [B]).  Rows shorter than
    cfg.min_frames have length 0; beyond a row's length the samples are zero; frames above T count as T."""
    mel = np.asarray(mel)
    B, T = mel.shape[:2]
    frames = np.full((B,), T) if frames is None else np.minimum(np.asarray(frames), T)
    wav = np.zeros((B, T * cfg.hop), dtype=dtype)
    lengths = np.zeros((B,), dtype=np.int32)
    for b in range(B):
        n = int(frames[b])
        if n < cfg.min_frames:
            continue
        wav[b, :n * cfg.hop] = melgan_row(cfg, weights, mel[b, :n].astype(dtype))
        lengths[b] = n * cfg.hop
    return wav, lengths


# ---------------------------------------------------------------------------------------------------- the plan's constants
def plan_tiles(cfg):
    """What gsttaco_melgan_plan reports as (kind, channels, tile, form, rate) per launch: the N-tiles a wave item owns by padded
    channel count, and the time tile that gives four waves an item each, halved while the launch's LDS does not fit
    (vocoder_cases.melgan_plan_rule)."""
    return [(s["kind"], s["channels"], s["tile"], s["form"], s["rate"]) for s in melgan_plan_rule(cfg)]


# ---------------------------------------------------------------------------------------------------- the cases
@dataclass
class Case:
    name: str
    cfg: melgan.MelGANConfig
    frames: tuple
    seed: int
    hot: bool = False

    @property
    def T(self):
        return max(max(self.frames), 1)

    @functools.cached_property
    def weights(self):
        w = melgan.synthetic_weights(self.cfg, seed=self.seed)
        if self.hot:
            # every hidden layer's bias pulled down, so most pre-activations are negative and the LeakyReLU's slope branch carries
            # the signal; the output conv scaled up until the tanh saturates on part of the waveform
            for name in w:
                if name.endswith("/bias") and name != "melgan/out/bias":
                    w[name] = (w[name] - 0.75).astype(np.float32)
            w["melgan/out/kernel"] = (w["melgan/out/kernel"] * 6.0).astype(np.float32)
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


_C = melgan.MelGANConfig
_EDGE = _C(mel_dim=5, base=4, ratios=[2, 2], n_res=3)           # min_frames 5: stage 1 has 10 samples for a reflection of 9
_TILES = _C(mel_dim=80, base=8)
CASES = {c.name: c for c in (
    Case("tiny", _C(mel_dim=5, base=4, ratios=[2, 2], n_res=2), (9, 5, 6), 1),
    Case("odd_channels", _C(mel_dim=7, base=3, ratios=[4, 2], n_res=3), (7, 5), 2),
    Case("min_rows", _EDGE, (_EDGE.min_frames, _EDGE.min_frames - 1, 0), 3),
    Case("dilation_edge", _EDGE, (5, 6), 4),
    Case("tiles", _TILES, tuple(tile_edge_frames(plan_tiles(_TILES), _TILES.min_frames)), 5),
    Case("full_size", _C(), (12, 7), 6),
    Case("hot", _C(mel_dim=8, base=4, ratios=[4, 2], n_res=2), (11, 6), 7, hot=True),
)}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float64"):
    """(wav, lengths) of a case, computed once and shared; callers leave it unchanged."""
    c = CASES[name]
    wav, lengths = melgan_reference(c.cfg, c.weights, c.mel, c.frames_array, dtype=np.dtype(dtype).type)
    wav.setflags(write=False)
    lengths.setflags(write=False)
    return wav, lengths


@functools.lru_cache(maxsize=None)
def e32(name):
    """max |float32 run - float64 run| of the restatement over the case"""
    return float(np.abs(reference(name, "float32")[0].astype(np.float64) - reference(name)[0]).max())
