"""The flow vocoder's float64 restatement and case table (tests/test_waveglow_cases.py admits the cases on the CPU,
tests/test_gpu_waveglow.py holds csrc/waveglow.hip to them).  ``waveglow_row`` is written from the contract in include/gsttaco.h
(gsttaco_waveglow_config), row by row at each row's own length, in NumPy; ``dtype=np.float32`` runs the same chain in float32, whose
distance from the float64 run (``e32``) is the yardstick of the device's error: both are fp32 chains of one depth that differ in
summation order and in the last ulps of tanh / sigmoid / exp only."""
import functools
from dataclasses import dataclass

import numpy as np

from gst_tacotron_amd import waveglow
from vocoder_cases import _conv as _conv_same     # (every WaveGlow conv has an odd tap count: 3 or 1)

MAX_ABS_MEL = 4.0
E32_MAX = 2.0 ** -14            # a case whose float32 run strays further from float64 is ill-conditioned: changed, not excused


# ---------------------------------------------------------------------------------------------------- the restatement
def _upsample(x, w, b, hop):
    """x [n, mel], w [win, mel, mel]: sample q hop + p sums taps p + j hop of frames q - j; cropped to n hop samples"""
    n, mel = x.shape
    up = np.tile(b[None, None, :], (n, hop, 1))
    for j in range(w.shape[0] // hop):
        if j < n:
            up[j:] = up[j:] + np.einsum("qc,pcm->qpm", x[:n - j], w[j * hop:(j + 1) * hop])
    return up.reshape(n * hop, mel)


def waveglow_row(cfg, w, x, z, sigma, used=None):
    """One row alone: x [frames >= 1, mel_dim], z [frames * hop] -> (wav [frames * hop], the largest |s|); the dtype is x's (the
    weights, z and sigma are cast to it).  ``used``: a list that receives the z columns in the order they are taken."""
    dt = x.dtype
    g = lambda name: np.asarray(w[name], dtype=dt)
    G, C, F = cfg.n_group, cfg.n_channels, cfg.n_flows
    n = x.shape[0]
    L = n * cfg.hop // G
    up = _upsample(x, g("waveglow/up/kernel"), g("waveglow/up/bias"), cfg.hop)
    spect = up.reshape(L, G, cfg.mel_dim).transpose(0, 2, 1).reshape(L, cfg.mel_dim * G)       # spect[l, m G + g] = up[l G + g, m]
    zz = np.asarray(z, dtype=dt).reshape(L, G)
    sigma = dt.type(sigma)
    chans = cfg.flow_channels()
    zcol = chans[-1]
    audio = sigma * zz[:, :zcol]
    if used is not None:
        used.extend(range(zcol))
    smax = 0.0
    for k in range(F - 1, -1, -1):
        p, h = f"waveglow/flow{k}/", chans[k] // 2
        a0, a1 = audio[:, :h], audio[:, h:]
        hid = _conv_same(a0, g(p + "start/kernel"), g(p + "start/bias"), 1, 1)
        out = np.zeros((L, C), dtype=dt)
        for i in range(cfg.n_layers):
            q = f"{p}layer{i}/"
            acts = _conv_same(hid, g(q + "in/kernel"), g(q + "in/bias"), 3, 2 ** i) + _conv_same(spect, g(q + "cond/kernel"), g(q + "cond/bias"), 1, 1)
            gate = np.tanh(acts[:, :C]) * (dt.type(1) / (dt.type(1) + np.exp(-acts[:, C:])))
            rs = _conv_same(gate, g(q + "res_skip/kernel"), g(q + "res_skip/bias"), 1, 1)
            if i < cfg.n_layers - 1:
                hid = hid + rs[:, :C]
                out = out + rs[:, C:]
            else:
                out = out + rs
        o = _conv_same(out, g(p + "end/kernel"), g(p + "end/bias"), 1, 1)
        b, s = o[:, :h], o[:, h:]
        smax = max(smax, float(np.abs(s).max()))
        a1 = (a1 - b) * np.exp(-s)
        winv = np.linalg.inv(np.asarray(w[p + "W"], dtype=np.float64)).astype(dt)              # float64 on the host, once, as at load
        audio = np.concatenate([a0, a1], axis=1) @ winv.T
        if k % cfg.n_early_every == 0 and k > 0:
            audio = np.concatenate([sigma * zz[:, zcol:zcol + cfg.n_early_size], audio], axis=1)
            if used is not None:
                used.extend(range(zcol, zcol + cfg.n_early_size))
            zcol += cfg.n_early_size
    return audio.reshape(L * G), smax


def waveglow_reference(cfg, weights, mel, frames, z, sigma, dtype=np.float64):
    """mel [B, T, mel_dim], frames [B] or None, z [B, T * hop] -> (wav [B, T * hop] of ``dtype``, lengths int32 [B], the largest |s|).
    Rows of fewer than 1 frame have length 0; beyond a row's length the samples are zero; frames above T count as T."""
    mel = np.asarray(mel)
    B, T = mel.shape[:2]
    frames = np.full((B,), T) if frames is None else np.minimum(np.asarray(frames), T)
    wav = np.zeros((B, T * cfg.hop), dtype=dtype)
    lengths = np.zeros((B,), dtype=np.int32)
    smax = 0.0
    for b in range(B):
        n = int(frames[b])
        if n < 1:
            continue
        wav[b, :n * cfg.hop], s = waveglow_row(cfg, weights, mel[b, :n].astype(dtype), np.asarray(z)[b, :n * cfg.hop], sigma)
        lengths[b] = n * cfg.hop
        smax = max(smax, s)
    return wav, lengths, smax


def tile_edge_frames(stages, hop):
    """One, zero and one more frame around the first and second multiple of each launch's time tile (``stages``: the dicts of
    gsttaco_waveglow_plan, or (tile, unit) pairs) that a whole frame count reaches."""
    frames = set()
    for s in stages:
        tile, unit = (s["tile"], s["unit"]) if isinstance(s, dict) else s
        for m in (1, 2):
            if (m * tile * unit) % hop == 0:
                f = m * tile * unit // hop
                frames.update(v for v in (f - 1, f, f + 1) if v >= 1)
    return sorted(frames)


# ---------------------------------------------------------------------------------------------------- the cases
@dataclass
class Case:
    name: str
    cfg: waveglow.WaveGlowConfig
    frames: tuple
    seed: int
    gain_s: float = 0.25
    sigma: float = 0.6

    @property
    def T(self):
        return max(max(self.frames), 1)

    @functools.cached_property
    def weights(self):
        return waveglow.synthetic_weights(self.cfg, seed=self.seed, gain_s=self.gain_s)

    @functools.cached_property
    def mel(self):
        rng = np.random.default_rng(1000 + self.seed)
        x = rng.uniform(-MAX_ABS_MEL, MAX_ABS_MEL, (len(self.frames), self.T, self.cfg.mel_dim))
        return x.astype(np.float32)         # (frames beyond a row's length hold values too: they must not be read)

    @functools.cached_property
    def z(self):
        rng = np.random.default_rng(2000 + self.seed)
        return rng.normal(0.0, 1.0, (len(self.frames), self.T * self.cfg.hop)).astype(np.float32)

    @property
    def frames_array(self):
        return np.asarray(self.frames, dtype=np.int32)


def _cfg(**kw):
    base = dict(mel_dim=8, hop=16, win=64, n_group=8, n_flows=4, n_early_every=2, n_early_size=2, n_layers=2, n_channels=16)
    base.update(kw)
    return waveglow.WaveGlowConfig(**base).check()


# the launches' (tile, unit) of _TILES in the order gsttaco_waveglow_plan first reports them (tests/test_waveglow_cases.py checks that it
# does): the upsampler's 64 frames of hop samples, the flow tail's 64 columns and the WN layer's 256 columns of n_group samples
_TILES = _cfg(mel_dim=80, hop=32, win=64, n_flows=2, n_channels=16)
TILES_PLAN = ((64, 32), (64, 8), (256, 8))
CASES = {c.name: c for c in (
    Case("tiny", _cfg(), (9, 1, 0, 5), 1),
    Case("odd_channels", _cfg(mel_dim=5, win=32, n_flows=3, n_layers=3, n_channels=24), (7, 4), 2),
    Case("dilation_edge", _cfg(n_flows=2, n_layers=5), (1, 2, 3), 3),
    Case("early_default", _cfg(win=32, n_flows=12, n_early_every=4), (5, 3), 4),
    Case("early_g4", _cfg(win=32, n_group=4, n_flows=3), (6, 2), 5),
    Case("early_g16", _cfg(hop=32, win=64, n_group=16), (4, 3), 6),
    Case("win_1", _cfg(win=16), (5, 2), 7),
    Case("win_2", _cfg(win=32), (5, 2), 8),
    Case("win_8", _cfg(win=128), (3, 2), 9),
    Case("tiles", _TILES, tuple(tile_edge_frames(TILES_PLAN, _TILES.hop)), 10),
    Case("full_size", waveglow.WaveGlowConfig(), (6, 3), 11),
    Case("hot", _cfg(n_layers=3), (7, 3), 12, gain_s=0.7, sigma=1.0),
)}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float64", sigma=None, zscale=1.0):
    """(wav, lengths, max |s|) of a case, computed once and shared; callers leave it unchanged.  ``sigma`` / ``zscale``: the case at
    another temperature / with its z scaled."""
    c = CASES[name]
    dt = np.dtype(dtype).type
    z = c.z if zscale == 1.0 else (c.z * np.float32(zscale)).astype(np.float32)
    wav, lengths, smax = waveglow_reference(c.cfg, c.weights, c.mel, c.frames_array, z, c.sigma if sigma is None else sigma, dtype=dt)
    wav.setflags(write=False)
    lengths.setflags(write=False)
    return wav, lengths, smax


@functools.lru_cache(maxsize=None)
def e32(name, sigma=None, zscale=1.0):
    """max |float32 run - float64 run| of the restatement over the case"""
    return float(np.abs(reference(name, "float32", sigma, zscale)[0].astype(np.float64) - reference(name, "float64", sigma, zscale)[0]).max())
