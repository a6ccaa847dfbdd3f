"""The size surface of the three neural vocoders (csrc/melgan.hip, hifigan.hip, waveglow.hip on csrc/vocoder_common.h): the widths at
which the four waves of a workgroup take UNEVEN numbers of items or idle through a phase whose barriers they still take part in, the
sizes at which a plan HALVES a time tile to fit the LDS (fewer items than waves, a halo wider than the tile), the launches at EXACTLY
the 163840 bytes a plan admits, and WaveGlow's K chunks of 64 and 16 and its one-workgroup-a-CU fallback.  The case tables of
tests/{melgan,hifigan,waveglow}_cases.py reach none of these: every MFMA launch of every case there has a multiple of four items, no
tile is shrunk and kc is 32.

tests/test_vocoder_surface_cases.py admits the rows on the CPU, holds the library's plans to vocoder_cases' restated rule and asserts
from the rows' own plans that the table reaches what it names; tests/test_gpu_vocoder_surface.py runs the rows on the GPU.  The rows
are NOT part of the modules' CASES tables (whose measured ratios stand in docstrings); tools/vocoder_bits.py hashes both.

Every number comes from the restatements the modules already pin against torch's own modules: ``melgan_reference``,
``hifigan_reference``, ``waveglow_reference`` in float64 and float32, ``hifigan_half_cases.launch_reference`` per launch.  Weights
are each module's ``synthetic_weights(cfg, seed)``; mels and z are the modules' own ``Case`` draws.

Frame counts: around the first and second multiple of the row's own tiles (shrunk ones included) that a frame count up to about
2 tile / rate reaches, a row of 0 frames, MelGAN's min_frames - 1 and min_frames; hg_shrunk also below, at and above each of its
dilations at its stage's rate of 2."""
import functools
from dataclasses import dataclass

import numpy as np

import hifigan_cases as HG
import hifigan_half_cases as H
import melgan_cases as MG
import vocoder_cases as V
import waveglow_cases as WG

E32_MAX = MG.E32_MAX            # the modules' admission rule, unchanged
RMS_MIN = 0.05                  # a row's waveform is not silent
SMAX = 4.0                      # tests/test_waveglow_cases.py's bound on the largest |s|

_M, _H = MG.melgan.MelGANConfig, HG.hifigan.HiFiGANConfig


@dataclass
class Row:
    module: str                 # "melgan", "hifigan" or "waveglow"
    case: object                # the module's own Case
    reach: tuple                # (kind, channels, tile, form, items) that some launch of the row's plan must have
    why: str

    @property
    def name(self):
        return self.case.name


def _mg(name, cfg, frames, seed, reach, why):
    return Row("melgan", MG.Case(name, cfg, frames, seed), reach, why)


def _hg(name, cfg, frames, seed, reach, why):
    return Row("hifigan", HG.Case(name, cfg, frames, seed), reach, why)


def _wg(name, kw, frames, seed, reach, why):
    return Row("waveglow", WG.Case(name, WG._cfg(**kw), frames, seed), reach, why)


# hg_shrunk: 16 channels at k = 11, rows of 80 bytes, 2048 of them in 163840 bytes.  d = 179: 256 + 1790 rows, the tile unshrunk at
# 163680 bytes; d = 192: 128 + 1920 = 2048 rows, shrunk once, EXACTLY the bound; d = 198: 64 + 1980 rows, shrunk twice, one item and
# three idle waves; d = 199 (64 + 1990 rows) is refused.  Its stage runs at rate 2: 89 / 90 frames are 178 / 180 samples around d = 179,
# 96 / 97 around 192, 99 / 100 around 198; 32, 64 and 128 frames end a tile of 64, 128 and 256.
_HG_SHRUNK = _H(mel_dim=5, initial=32, rates=[2], resblock=2, kernels=[11], dilations=[[179, 192, 198]])
# mg_shrunk: 96 channels, rows of 400 bytes.  Block 4 (d = 81): 2 x 128 + 162 rows are 167200 bytes, so its tile is 64: three items for
# four waves, and a halo of 81 rows each side, wider than the tile.  Blocks 0 .. 3 (d <= 27) keep 128.  min_frames is 41.
_MG_SHRUNK = _M(mel_dim=5, base=96, ratios=[2], n_res=5)

ROWS = {r.name: r for r in (
    _mg("mg_96_48", _M(mel_dim=7, base=24, ratios=[2, 2], n_res=2), (0, 3, 4, 63, 64, 65, 129), 21,
        (("in", 96, 128, 2, 6), ("up", 48, 128, 1, 12), ("res", 48, 128, 1, 6), ("res", 24, 256, 2, 4)),
        "six items for four waves at form 2 and at form 1: waves 0 and 1 take two, waves 2 and 3 one"),
    _mg("mg_160_80_48", _M(mel_dim=7, base=40, ratios=[4, 2], n_res=2), (0, 3, 4, 16, 17, 33, 65), 22,
        (("in", 160, 64, 2, 5), ("res", 80, 64, 1, 5), ("up", 40, 128, 1, 12), ("res", 40, 128, 1, 6)),
        "five groups: wave 0 alone takes a second item; 40 channels pad to 48, three groups on two M-groups"),
    _mg("mg_320", _M(mel_dim=7, base=80, ratios=[2, 2], n_res=2), (0, 3, 4, 17, 32, 33, 65), 23,
        (("in", 320, 64, 4, 5), ("res", 160, 64, 2, 5), ("res", 80, 64, 1, 5)),
        "form 4 with five groups, the only odd group count form 4 meets"),
    _mg("mg_112", _M(mel_dim=7, base=28, ratios=[2, 2], n_res=2), (0, 3, 4, 31, 33, 64, 65), 24,
        (("in", 112, 64, 1, 7),),
        "seven items: three waves take two, wave 3 one"),
    _mg("mg_shrunk", _MG_SHRUNK, (0, 40, 41, 64, 65, 97), 25,
        (("res", 96, 64, 2, 3), ("res", 96, 128, 2, 6), ("in", 192, 64, 2, 6)),
        "the residual block's tile halved once: three items, wave 3 idle between the block's two barriers, halo 81 > tile 64"),
    _hg("hg_96", _H(mel_dim=7, initial=96, rates=[2, 2], resblock=1, kernels=[3, 7], dilations=[[1, 3], [2]]), (0, 1, 33, 64, 65, 129), 31,
        (("in", 96, 128, 2, 6), ("conv", 48, 128, 1, 6), ("conv", 24, 256, 2, 4)),
        "six items; 48 channels are 64 in the 16-bit forms' rows"),
    _hg("hg_160", _H(mel_dim=7, initial=160, rates=[2, 2], resblock=2, kernels=[3, 5], dilations=[[1, 3], [2]]), (0, 1, 16, 31, 32, 33, 65), 32,
        (("in", 160, 64, 2, 5), ("conv", 80, 64, 1, 5), ("conv", 40, 128, 1, 6)),
        "five items; 80 channels are 96 in the 16-bit forms' rows"),
    _hg("hg_320", _H(mel_dim=7, initial=320, rates=[2, 2], resblock=2, kernels=[3], dilations=[[1, 3]]), (0, 1, 15, 16, 17, 33, 65), 33,
        (("in", 320, 64, 4, 5), ("conv", 160, 64, 2, 5), ("conv", 80, 64, 1, 5)),
        "form 4 with five groups"),
    _hg("hg_224", _H(mel_dim=7, initial=224, rates=[2], resblock=1, kernels=[3], dilations=[[2]]), (0, 1, 31, 32, 33, 64, 65), 34,
        (("in", 224, 64, 2, 7), ("conv", 112, 64, 1, 7)),
        "seven items at form 2 and at form 1; 112 channels are 128 in the 16-bit forms' rows"),
    _hg("hg_shrunk", _HG_SHRUNK, (0, 1, 32, 33, 64, 65, 89, 90, 96, 97, 99, 100, 128, 129, 200), 35,
        (("conv", 16, 256, 1, 4), ("conv", 16, 128, 1, 2), ("conv", 16, 64, 1, 1)),
        "a tile unshrunk just below the bound, one halved once to EXACTLY 163840 bytes (in all three operand forms: 20 floats and 40 "
        "halves are both 80 bytes), one halved twice: one item, three waves idle, a halo of 1980 rows around 64"),
    _wg("wg_c48", dict(n_channels=48), (0, 1, 33, 63, 64, 65, 128), 41,
        (("layer", 48, 128, 2, 6),),
        "six gate items in two passes: in the second, waves 2 and 3 are inactive and still stage and wait; kc 64"),
    _wg("wg_c80", dict(n_channels=80), (0, 1, 31, 32, 33, 64, 65), 42,
        (("layer", 80, 64, 2, 5),),
        "five gate items; kc 64 under C_p = 80: the hidden state's K loop runs a chunk of 64 and a partial one of 16"),
    _wg("wg_c96", dict(n_channels=96, mel_dim=5), (0, 1, 33, 64, 65, 127), 43,
        (("layer", 96, 128, 4, 6),),
        "form 4 with three groups; kc 32; spect 40 channels in 48"),
    _wg("wg_c64", dict(n_channels=64), (0, 1, 65, 127, 128, 129), 44,
        (("layer", 64, 256, 8, 4),),
        "form 8 at tile 256: no K chunk lets two workgroups share a CU, so kc 64 at one workgroup a CU (139264 bytes)"),
    _wg("wg_c128", dict(n_channels=128), (0, 2, 63, 64, 65, 128), 45,
        (("layer", 128, 128, 8, 4),),
        "kc 16, the narrowest chunk (77824 bytes twice a CU)"),
    _wg("wg_win_1794", dict(win=16 * 1794, n_flows=2), (5, 2, 0, 3), 46,
        (("up", 8, 128, 1, 32),),
        "the upsampler's tile halved once (256 + 1793 rows of 80 bytes do not fit): 153680 bytes"),
    _wg("wg_win_1793", dict(win=16 * 1793, n_flows=2), (5, 2, 0, 3), 47,
        (("up", 8, 256, 1, 64),),
        "the upsampler's tile unshrunk at EXACTLY 163840 bytes: 256 + 1792 rows"),
    _wg("wg_win_1985", dict(win=16 * 1985, n_flows=2), (5, 2, 0, 3), 48,
        (("up", 8, 64, 1, 16),),
        "the upsampler's tile halved twice, at EXACTLY 163840 bytes: 64 + 1984 rows"),
)}
NAMES = tuple(ROWS)
MODULE_NAMES = {m: tuple(n for n in NAMES if ROWS[n].module == m) for m in ("melgan", "hifigan", "waveglow")}
# the rows that carry the bitwise promises and the NaN test on the GPU, and HiFi-GAN's 16-bit rows
BITWISE = ("mg_160_80_48", "mg_shrunk", "hg_224", "hg_shrunk", "wg_c48", "wg_c80", "wg_c64")
NAN_BEYOND = ("mg_shrunk", "hg_shrunk", "wg_c48")
HALF = ("hg_96", "hg_160", "hg_224", "hg_shrunk")
EXACT_BOUND = ("hg_shrunk", "wg_win_1793", "wg_win_1985")      # rows with a launch at exactly V.LDS_MAX bytes

# One step past an admitted row: (module, configuration, the field the refusal names)
REFUSED = (
    ("melgan", _M(mel_dim=5, base=96, ratios=[2], n_res=6), "residual blocks"),
    ("hifigan", _H(mel_dim=5, initial=32, rates=[2], resblock=2, kernels=[11], dilations=[[199]]), "dilations"),
    ("waveglow", WG._cfg(win=16 * 1986, n_flows=2), "win"),
)


def rule_plan(row_or_module, cfg=None, operands="float32"):
    """The restated plan of a row (or of (module, cfg)): the list of MelGAN's / HiFi-GAN's launches; for WaveGlow its two MFMA launches."""
    module, cfg = (row_or_module.module, row_or_module.case.cfg) if cfg is None else (row_or_module, cfg)
    if module == "melgan":
        return V.melgan_plan_rule(cfg)
    if module == "hifigan":
        return V.hifigan_plan_rule(cfg, operands)
    p = V.waveglow_plan_rule(cfg)
    return None if p is None else [p["up"], p["layer"]]


# ---------------------------------------------------------------------------------------------------- references, computed once
@functools.lru_cache(maxsize=None)
def reference(name, dtype="float64"):
    """(wav, lengths) of a row's case, computed once and shared; callers leave it unchanged.  WaveGlow: with the case's z; the third
    entry is the largest |s|."""
    r = ROWS[name]
    c, dt = r.case, np.dtype(dtype).type
    if r.module == "melgan":
        out = MG.melgan_reference(c.cfg, c.weights, c.mel, c.frames_array, dtype=dt)
    elif r.module == "hifigan":
        out = HG.hifigan_reference(c.cfg, c.weights, c.mel, c.frames_array, dtype=dt)
    else:
        out = WG.waveglow_reference(c.cfg, c.weights, c.mel, c.frames_array, c.z, c.sigma, dtype=dt)
    for a in out[:2]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def e32(name):
    """max |float32 run - float64 run| of the restatement over the row's case"""
    return float(np.abs(reference(name, "float32")[0].astype(np.float64) - reference(name)[0]).max())


@functools.lru_cache(maxsize=None)
def half_reference(name, precision):
    c = ROWS[name].case
    wav = H.half_reference(c.cfg, c.weights, c.mel, c.frames_array, precision)
    wav.setflags(write=False)
    return wav


@functools.lru_cache(maxsize=None)
def e_h(name, precision):
    """max |rounded-operand float64 run - exact float64 run| over a HiFi-GAN row (hifigan_half_cases.e_h for a row of this table)"""
    return float(np.abs(half_reference(name, precision) - reference(name)[0]).max())


# ---------------------------------------------------------------------------------------------------- mutations of the oracle
def melgan_row_tiled(cfg, w, x, skip_last_item_of_in=None, res_reflect_at=None):
    """``melgan_cases.melgan_row`` with two of the bugs this table exists for put in ON THE ORACLE'S SIDE; with neither it is
    melgan_row bit for bit.
      skip_last_item_of_in = (tile, form): the input conv's last wave item (the last ``form`` N-tiles) is skipped: its output columns
        stay at the bias, as they do when a strided item loop ends one item early.
      res_reflect_at = (stage, block, tile): that residual block's dilated conv reflects at the END OF ITS TILE where the row goes on
        beyond it, as a bound taken at the tile instead of at the row does."""
    dt = x.dtype
    slope = dt.type(cfg.slope)
    g = lambda name: np.asarray(w[name], dtype=dt)
    h = MG._conv(MG._reflect(x, 3), g("melgan/in/kernel"), g("melgan/in/bias"), 7, 1)
    if skip_last_item_of_in is not None:
        tile, form = skip_last_item_of_in
        first = (V._pad16(h.shape[1]) // 16 // form - 1) * form * 16
        h[:, first:] = g("melgan/in/bias")[None, first:]
    for i, r in enumerate(cfg.ratios):
        h = MG._transposed(MG._leaky(h, slope), g(f"melgan/up{i}/kernel"), g(f"melgan/up{i}/bias"), r)
        for j in range(cfg.n_res):
            p, d = f"melgan/up{i}/res{j}/", 3 ** j
            a = MG._leaky(h, slope)
            if res_reflect_at is not None and res_reflect_at[:2] == (i, j):
                tile, L = res_reflect_at[2], h.shape[0]
                t = np.empty_like(h)
                for t0 in range(0, L, tile):
                    end = min(t0 + tile, L)
                    pos = np.arange(t0 - d, end + d)
                    pos = np.abs(np.where(pos < 0, -pos, np.where(pos >= end, 2 * (end - 1) - pos, pos)))
                    t[t0:end] = MG._conv(a[pos], g(p + "conv3/kernel"), g(p + "conv3/bias"), 3, d)
            else:
                t = MG._conv(MG._reflect(a, d), g(p + "conv3/kernel"), g(p + "conv3/bias"), 3, d)
            t = MG._conv(MG._leaky(t, slope), g(p + "conv1/kernel"), g(p + "conv1/bias"), 1, 1)
            h = MG._conv(h, g(p + "shortcut/kernel"), g(p + "shortcut/bias"), 1, 1) + t
    y = MG._conv(MG._reflect(MG._leaky(h, slope), 3), g("melgan/out/kernel"), g("melgan/out/bias"), 7, 1)
    return np.tanh(y[:, 0])
