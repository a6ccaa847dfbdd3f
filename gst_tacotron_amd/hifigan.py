"""The HiFi-GAN vocoder's host side: the generator's configuration (V1 / V2 / V3 and anything of their shape), weight manifest, a
seeded synthetic initialiser and the loader for the public checkpoint layout (Kong, Kim & Bae 2020: ``Generator`` of the public
implementation -- ``conv_pre``, ``ups``, ``resblocks``, ``conv_post``, weight-normalised).  The network itself is stated in
include/gsttaco.h (gsttaco_hifigan_config) and runs in csrc/hifigan.hip; nothing here computes it.

Weights are named, plain (weight norm folded) float32 arrays in the project's ``[taps * cin, cout]`` convention:
``hifigan/in/kernel``, ``hifigan/up<i>/kernel`` ([2u, cin, cout]), ``hifigan/up<i>/res<j>/unit<m>/conv1/kernel`` (the conv at the
unit's dilation) and, under ``resblock = 1``, ``.../conv2/kernel`` (the unit's closing conv at dilation 1), ``hifigan/out/kernel``,
each with ``.../bias``.

``round_operand`` states, in NumPy, the one rounding the optional 16-bit operand forms apply (``Load_HiFiGAN(precision=)``, the
section's ``Precision`` key, ``gsttaco_hifigan_set_operands``): the two operands of each matrix product, nothing else.

The loader's layout is NOT verified against a trained public checkpoint (none is at hand): it is pinned to torch's own modules,
built as the public generator, on the CPU (tests/test_hifigan_cases.py).  Public checkpoints were trained on natural-log mels at
another scale than this project's normalised ones and will not sound right here; the use is a vocoder trained on ``Inference_GTA``
output.
"""
from dataclasses import dataclass, field
from typing import List

import numpy as np

from . import vocoder_common
from .vocoder_common import _np, conv_kernel, fold_weight_norm      # (fold_weight_norm: part of this module's interface)


@dataclass
class HiFiGANConfig:
    mel_dim: int = 80
    initial: int = 512
    rates: List[int] = field(default_factory=lambda: [8, 8, 2, 2])
    resblock: int = 1
    kernels: List[int] = field(default_factory=lambda: [3, 7, 11])
    dilations: List[List[int]] = field(default_factory=lambda: [[1, 3, 5], [1, 3, 5], [1, 3, 5]])
    slope: float = 0.1
    out_slope: float = 0.01         # the public code's F.leaky_relu default in front of conv_post, not ``slope``

    @property
    def hop(self):
        return int(np.prod(self.rates, dtype=np.int64))

    @property
    def min_frames(self):
        """Zero padding needs no length: one frame is enough."""
        return 1

    def channels(self):
        """Channels behind the input conv and behind every rate."""
        return [self.initial >> i for i in range(len(self.rates) + 1)]

    @classmethod
    def v1(cls, mel_dim=80):
        return cls(mel_dim=mel_dim)

    @classmethod
    def v2(cls, mel_dim=80):
        return cls(mel_dim=mel_dim, initial=128)

    @classmethod
    def v3(cls, mel_dim=80):
        return cls(mel_dim=mel_dim, initial=256, rates=[8, 8, 4], resblock=2, kernels=[3, 5, 7], dilations=[[1, 2], [2, 6], [3, 12]])


PRECISIONS = ("float32", "bfloat16", "float16")


def check_precision(precision):
    if precision not in PRECISIONS:
        raise ValueError("precision must be 'float32', 'bfloat16' or 'float16', not {!r}".format(precision))
    return precision


def precision_from_hp(hp):
    """The section's optional ``Precision`` key (the operand type of the matrix products), "float32" where it or the section is absent."""
    return check_precision((hp.get("Vocoder_HiFiGAN") or {}).get("Precision") or "float32")


def round_operand(x, precision):
    """What ``gsttaco_hifigan_set_operands`` does to an operand of a matrix product, stated on the host: ``x`` (any float array) is
    rounded once to ``precision`` and returned in x's own dtype (every bfloat16 and float16 is exact in float32 and float64).
    "float32" returns x unchanged.  "bfloat16": to nearest, ties to even, on the float32 bits (a float64 x is first rounded to
    float32, as the device only ever sees float32); NaN stays NaN.  "float16": clipped to +-65504 (the device saturates where the
    plain conversion would give inf), then ``np.float16``'s conversion, nearest even with subnormals."""
    check_precision(precision)
    x = np.asarray(x)
    if precision == "float32":
        return x
    if precision == "float16":
        return np.clip(x, -65504.0, 65504.0).astype(np.float16).astype(x.dtype)
    f = np.ascontiguousarray(x, dtype=np.float32)
    u = f.view(np.uint32)
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    r = np.where(np.isnan(f), (u & np.uint32(0xFFFF0000)) | np.uint32(0x00400000), r).astype(np.uint32)
    return r.view(np.float32).reshape(x.shape).astype(x.dtype)


def from_hp(hp):
    """The configuration of Hyper_Parameters' optional ``Vocoder_HiFiGAN`` section (V1 where a key is absent), or None without it.
    The section's ``Precision`` and ``Checkpoint_Path`` are no part of the network: see ``precision_from_hp``."""
    sec = hp.get("Vocoder_HiFiGAN")
    if sec is None:
        return None
    d = HiFiGANConfig()
    return HiFiGANConfig(mel_dim=int(hp["Sound"]["Mel_Dim"]), initial=int(sec.get("Initial_Filters", d.initial)),
                         rates=[int(r) for r in sec.get("Upsample_Rates", d.rates)], resblock=int(sec.get("Resblock", d.resblock)),
                         kernels=[int(k) for k in sec.get("Resblock_Kernel_Sizes", d.kernels)],
                         dilations=[[int(v) for v in row] for row in sec.get("Resblock_Dilation_Sizes", d.dilations)],
                         slope=float(sec.get("Leaky_Slope", d.slope)), out_slope=float(sec.get("Output_Leaky_Slope", d.out_slope)))


def manifest(cfg):
    """Ordered dict name -> shape, as gsttaco_hifigan_weight_info reports it."""
    ch = cfg.channels()
    m = {"hifigan/in/kernel": (7 * cfg.mel_dim, ch[0]), "hifigan/in/bias": (ch[0],)}
    for i, r in enumerate(cfg.rates):
        cin, c = ch[i], ch[i + 1]
        m[f"hifigan/up{i}/kernel"] = (2 * r, cin, c)
        m[f"hifigan/up{i}/bias"] = (c,)
        for j, (k, dils) in enumerate(zip(cfg.kernels, cfg.dilations)):
            for u in range(len(dils)):
                for leaf in ("conv1", "conv2")[:2 if cfg.resblock == 1 else 1]:
                    m[f"hifigan/up{i}/res{j}/unit{u}/{leaf}/kernel"] = (k * c, c)
                    m[f"hifigan/up{i}/res{j}/unit{u}/{leaf}/bias"] = (c,)
    m["hifigan/out/kernel"] = (7 * ch[-1], 1)
    m["hifigan/out/bias"] = (1,)
    return m


def synthetic_weights(cfg, seed=0, gain=1.0):
    """Seeded synthetic weights under which activations stay O(1) through every stage for O(1) mels: normal kernels of variance
    share / (fan_in * E[LeakyReLU(z)^2]) -- fan_in the taps an output actually sums (two for the transposed conv) times the input
    channels, the second moment of LeakyReLU 0.5 (1 + slope^2).  The first conv of a unit has share 1; a unit's closing conv (under
    ``resblock = 2`` its only conv) has share 0.25, so that a residual chain of up to four units adds about the variance it started
    with; biases ~ N(0, 0.05).  The output conv, behind the output slope, lands at a pre-tanh variance of about one: the waveform
    neither vanishes nor saturates.  ``gain`` scales every kernel."""
    rng = np.random.default_rng(seed)
    act = 0.5 * (1.0 + cfg.slope * cfg.slope)
    act_out = 0.5 * (1.0 + cfg.out_slope * cfg.out_slope)
    w = {}
    for name, shape in manifest(cfg).items():
        parts = name.split("/")
        if parts[-1] == "bias":
            a = rng.normal(0.0, 0.05, shape)
        else:
            leaf = parts[-2]
            if leaf == "in":
                var = 1.0 / shape[0]
            elif leaf.startswith("up"):
                var = 1.0 / (2 * shape[1] * act)
            elif leaf == "conv1" and cfg.resblock == 1:
                var = 1.0 / (shape[0] * act)
            elif leaf in ("conv1", "conv2"):
                var = 0.25 / (shape[0] * act)
            else:
                var = 1.0 / (shape[0] * act_out)
            a = rng.normal(0.0, gain * np.sqrt(var), shape)
        w[name] = np.require(np.asarray(a, dtype=np.float32), requirements="C").reshape(shape)
    return w


def check_weights(cfg, weights):
    vocoder_common.check_weights(manifest(cfg), weights)


def infer_config(weights, dilations=None, slope=0.1, out_slope=0.01):
    """The configuration a set of named arrays was made for.  The arrays' shapes say everything but the dilations: without
    ``dilations`` they are the shipped ones where the rest has a shipped shape (kernels 3 / 7 / 11 with three units under
    ``resblock = 1``: [1, 3, 5] each; kernels 3 / 5 / 7 with two units under ``resblock = 2``: [1, 2], [2, 6], [3, 12]); anything
    else must name them."""
    rates = []
    while f"hifigan/up{len(rates)}/kernel" in weights:
        rates.append(int(np.shape(weights[f"hifigan/up{len(rates)}/kernel"])[0]) // 2)
    if not rates:
        raise ValueError("not HiFi-GAN weights: no hifigan/up0/kernel")
    resblock = 1 if "hifigan/up0/res0/unit0/conv2/kernel" in weights else 2
    c = int(np.shape(weights["hifigan/up0/kernel"])[2])
    kernels, units = [], []
    while f"hifigan/up0/res{len(kernels)}/unit0/conv1/kernel" in weights:
        j = len(kernels)
        kernels.append(int(np.shape(weights[f"hifigan/up0/res{j}/unit0/conv1/kernel"])[0]) // c)
        n = 0
        while f"hifigan/up0/res{j}/unit{n}/conv1/kernel" in weights:
            n += 1
        units.append(n)
    if dilations is None:
        if resblock == 1 and kernels == [3, 7, 11] and units == [3, 3, 3]:
            dilations = [[1, 3, 5]] * 3
        elif resblock == 2 and kernels == [3, 5, 7] and units == [2, 2, 2]:
            dilations = [[1, 2], [2, 6], [3, 12]]
        else:
            raise ValueError("the dilations cannot be read off the weights' shapes and this is no shipped shape: pass dilations= or a config")
    dilations = [[int(v) for v in row] for row in dilations]
    if [len(row) for row in dilations] != units:
        raise ValueError("dilations {} do not match the weights' units per kernel {}".format(dilations, units))
    return HiFiGANConfig(mel_dim=int(np.shape(weights["hifigan/in/kernel"])[0]) // 7, initial=int(np.shape(weights["hifigan/in/kernel"])[1]),
                         rates=rates, resblock=resblock, kernels=kernels, dilations=dilations, slope=slope, out_slope=out_slope)


def _layer(sd, prefix):
    """(plain float64 weight, float64 bias) of the layer ``prefix`` in any of the three spellings, or None where it is absent."""
    if prefix + ".weight" in sd:
        w = np.asarray(_np(sd[prefix + ".weight"]), dtype=np.float64)
    elif prefix + ".weight_g" in sd:
        w = fold_weight_norm(_np(sd[prefix + ".weight_g"]), _np(sd[prefix + ".weight_v"]))
    elif prefix + ".parametrizations.weight.original0" in sd:
        w = fold_weight_norm(_np(sd[prefix + ".parametrizations.weight.original0"]), _np(sd[prefix + ".parametrizations.weight.original1"]))
    else:
        return None
    if w.ndim != 3 or prefix + ".bias" not in sd:
        raise ValueError("layer '{}' is not a 1-D convolution with a bias".format(prefix))
    return w, np.asarray(_np(sd[prefix + ".bias"]), dtype=np.float64)


def from_state_dict(sd, dtype=np.float32):
    """The project's named, folded arrays of a public-layout generator ``state_dict``, read by name: ``conv_pre``, ``ups.<i>``,
    ``resblocks.<i * n_k + j>`` with ``convs1.<m>`` / ``convs2.<m>`` (ResBlock1) or ``convs.<m>`` (ResBlock2), ``conv_post``; each
    layer as ``weight_g`` / ``weight_v``, as plain ``weight`` (after ``remove_weight_norm``), or as torch's newer
    ``parametrizations.weight.original0`` / ``original1``; bare or under ``"generator"``.  Conv1d weights are [cout, cin, k],
    ConvTranspose1d weights [cin, cout, k].  The sizes are read off the shapes (the dilations are not in a state_dict: see
    ``infer_config``).  ``dtype``: the arrays' type (float64 keeps the folding's full precision)."""
    if "generator" in sd and isinstance(sd["generator"], dict):
        sd = sd["generator"]

    conv = lambda w: conv_kernel(w, dtype)

    pre, post = _layer(sd, "conv_pre"), _layer(sd, "conv_post")
    if pre is None or post is None:
        raise ValueError("not a HiFi-GAN generator: conv_pre / conv_post are missing")
    if pre[0].shape[2] != 7 or post[0].shape[2] != 7 or post[0].shape[0] != 1:
        raise ValueError("not a HiFi-GAN generator: conv_pre and conv_post must have 7 taps, conv_post one output channel")
    out = {"hifigan/in/kernel": conv(pre[0]), "hifigan/in/bias": pre[1].astype(dtype)}
    ups = []
    while _layer(sd, "ups.{}".format(len(ups))) is not None:
        ups.append(_layer(sd, "ups.{}".format(len(ups))))
    blocks = 0
    while any(k.startswith("resblocks.{}.".format(blocks)) for k in sd):
        blocks += 1
    if not ups or blocks == 0 or blocks % len(ups):
        raise ValueError("not a HiFi-GAN generator: {} ups, {} resblocks".format(len(ups), blocks))
    n_k = blocks // len(ups)
    for i, (w, b) in enumerate(ups):
        if w.shape[2] % 2 or w.shape[0] != 2 * w.shape[1]:
            raise ValueError("layer 'ups.{}': expected a ConvTranspose1d [cin, cin / 2, 2u], got {}".format(i, w.shape))
        out[f"hifigan/up{i}/kernel"] = np.ascontiguousarray(w.transpose(2, 0, 1), dtype=dtype)      # [k, cin, cout]
        out[f"hifigan/up{i}/bias"] = b.astype(dtype)
        for j in range(n_k):
            p = "resblocks.{}.".format(i * n_k + j)
            two = _layer(sd, p + "convs1.0") is not None
            m = 0
            while True:
                first = _layer(sd, p + ("convs1." if two else "convs.") + str(m))
                if first is None:
                    break
                pairs = [("conv1", first)]
                if two:
                    second = _layer(sd, p + "convs2." + str(m))
                    if second is None:
                        raise ValueError("'{}convs2.{}' is missing".format(p, m))
                    pairs.append(("conv2", second))
                for leaf, (wc, bc) in pairs:
                    if wc.shape[0] != wc.shape[1] or wc.shape[0] != w.shape[1] or not wc.shape[2] & 1:
                        raise ValueError("'{}': expected a residual conv [C, C, odd k] at C = {}, got {}".format(p + leaf, w.shape[1], wc.shape))
                    out[f"hifigan/up{i}/res{j}/unit{m}/{leaf}/kernel"] = conv(wc)
                    out[f"hifigan/up{i}/res{j}/unit{m}/{leaf}/bias"] = bc.astype(dtype)
                m += 1
            if m == 0:
                raise ValueError("'{}' has neither convs1 nor convs".format(p))
    out["hifigan/out/kernel"] = conv(post[0])
    out["hifigan/out/bias"] = post[1].astype(dtype)
    return out


def load(path):
    """A generator checkpoint in the public layout (``torch.save`` of its ``state_dict``, bare or under ``"generator"``) -> named,
    folded arrays.  ``state_dict``s only."""
    # (the strict loader of the three: weights_only, and a file without a dict is refused here; "generator" is unwrapped by from_state_dict)
    return from_state_dict(vocoder_common.load_state_dict(path, weights_only=True, refuse="'{}' does not hold a state_dict"))
