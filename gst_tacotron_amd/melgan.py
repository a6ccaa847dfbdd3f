"""The neural vocoder's host side: the MelGAN generator's configuration, weight manifest, a seeded synthetic initialiser and
the loader for the public checkpoint layout (Kumar et al. 2019: ``Generator`` of the public implementation, an ``nn.Sequential``
of weight-normalised Conv1d / ConvTranspose1d layers).  The network itself is stated in include/gsttaco.h (gsttaco_melgan_config)
and runs in csrc/melgan.hip; nothing here computes it.

Weights are named, plain (weight norm folded) float32 arrays in the project's ``[taps * cin, cout]`` convention:
``melgan/in/kernel``, ``melgan/up<i>/kernel`` ([2r, cin, cout]), ``melgan/up<i>/res<j>/{conv3,conv1,shortcut}/kernel``,
``melgan/out/kernel``, each with ``.../bias``.

The loader's layout is NOT verified against a trained public checkpoint (none is at hand): it is pinned to torch's own modules,
built in the public generator's layer order, on the CPU (tests/test_melgan_cases.py).
"""
from dataclasses import dataclass, field
from typing import List

import numpy as np

from . import vocoder_common
from .vocoder_common import _np, conv_kernel, fold_weight_norm      # (fold_weight_norm: part of this module's interface)


@dataclass
class MelGANConfig:
    mel_dim: int = 80
    base: int = 32
    ratios: List[int] = field(default_factory=lambda: [8, 8, 2, 2])
    n_res: int = 3
    slope: float = 0.2

    @property
    def hop(self):
        return int(np.prod(self.ratios, dtype=np.int64))

    @property
    def min_frames(self):
        """Rows shorter than this get length 0: reflection needs pad < length, for the input conv's pad of 3 and for the widest
        dilation 3^(n_res-1) at the first stage."""
        return max(4, 3 ** (self.n_res - 1) // self.ratios[0] + 1)

    def channels(self):
        """Channels behind the input conv and behind every ratio."""
        c = self.base << len(self.ratios)
        return [c >> i for i in range(len(self.ratios) + 1)]


def from_hp(hp):
    """The configuration of Hyper_Parameters' optional ``Vocoder_MelGAN`` section, or None without it."""
    sec = hp.get("Vocoder_MelGAN")
    if sec is None:
        return None
    return MelGANConfig(mel_dim=int(hp["Sound"]["Mel_Dim"]), base=int(sec.get("Base_Filters", 32)),
                        ratios=[int(r) for r in sec.get("Upsample_Ratios", [8, 8, 2, 2])], n_res=int(sec.get("Residual_Layers", 3)),
                        slope=float(sec.get("Leaky_Slope", 0.2)))


def manifest(cfg):
    """Ordered dict name -> shape, as gsttaco_melgan_weight_info reports it."""
    ch = cfg.channels()
    m = {"melgan/in/kernel": (7 * cfg.mel_dim, ch[0]), "melgan/in/bias": (ch[0],)}
    for i, r in enumerate(cfg.ratios):
        cin, c = ch[i], ch[i + 1]
        m[f"melgan/up{i}/kernel"] = (2 * r, cin, c)
        m[f"melgan/up{i}/bias"] = (c,)
        for j in range(cfg.n_res):
            for leaf, taps in (("conv3", 3), ("conv1", 1), ("shortcut", 1)):
                m[f"melgan/up{i}/res{j}/{leaf}/kernel"] = (taps * c, c)
                m[f"melgan/up{i}/res{j}/{leaf}/bias"] = (c,)
    m["melgan/out/kernel"] = (7 * cfg.base, 1)
    m["melgan/out/bias"] = (1,)
    return m


def synthetic_weights(cfg, seed=0, gain=1.0):
    """Seeded synthetic weights under which activations stay O(1) through every stage for O(1) mels: normal kernels of variance
    share / (fan_in * E[LeakyReLU(z)^2]) -- fan_in the taps an output actually sums (two for the transposed conv) times the input
    channels, the second moment of LeakyReLU 0.5 (1 + slope^2) where the layer is fed through one -- with the residual block's
    variance split evenly between the shortcut and the conv branch, and biases ~ N(0, 0.05).  The output conv lands at a
    pre-tanh variance of about one: the waveform neither vanishes nor saturates.  ``gain`` scales every kernel."""
    rng = np.random.default_rng(seed)
    act = 0.5 * (1.0 + cfg.slope * cfg.slope)
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
            elif leaf == "conv3":
                var = 1.0 / (shape[0] * act)
            elif leaf == "conv1":
                var = 0.5 / (shape[0] * act)
            elif leaf == "shortcut":
                var = 0.5 / shape[0]
            else:
                var = 1.0 / (shape[0] * act)
            a = rng.normal(0.0, gain * np.sqrt(var), shape)
        w[name] = np.require(np.asarray(a, dtype=np.float32), requirements="C").reshape(shape)
    return w


def check_weights(cfg, weights):
    vocoder_common.check_weights(manifest(cfg), weights)


def infer_config(weights, slope=0.2):
    """The configuration a set of named arrays was made for."""
    ratios = []
    while f"melgan/up{len(ratios)}/kernel" in weights:
        ratios.append(int(np.shape(weights[f"melgan/up{len(ratios)}/kernel"])[0]) // 2)
    n_res = 0
    while f"melgan/up0/res{n_res}/conv3/kernel" in weights:
        n_res += 1
    return MelGANConfig(mel_dim=int(np.shape(weights["melgan/in/kernel"])[0]) // 7, base=int(np.shape(weights["melgan/out/kernel"])[0]) // 7,
                        ratios=ratios, n_res=n_res, slope=slope)


def from_state_dict(sd, dtype=np.float32):
    """The project's named, folded float32 arrays of a public-layout generator ``state_dict``: a mapping whose entries come in layer
    order -- the input conv, then per ratio the transposed conv and its residual blocks (each block's dilated conv, its 1-tap conv,
    its shortcut), then the output conv -- as ``<layer>.weight_g`` / ``<layer>.weight_v`` / ``<layer>.bias``, or already folded as
    ``<layer>.weight``.  Conv1d weights are [cout, cin, k], ConvTranspose1d weights [cin, cout, k].  The sizes (ratios, residual
    blocks, channels) are read off the shapes.  ``dtype``: the arrays' type (float64 keeps the folding's full precision)."""
    layers, order = {}, []
    for key, value in sd.items():
        prefix, _, leaf = key.rpartition(".")
        if leaf not in ("weight_g", "weight_v", "weight", "bias"):
            continue
        if prefix not in layers:
            layers[prefix] = {}
            order.append(prefix)
        layers[prefix][leaf] = _np(value)
    seq = []
    for prefix in order:
        e = layers[prefix]
        if "weight" in e:
            w = np.asarray(e["weight"], dtype=np.float64)
        elif "weight_g" in e and "weight_v" in e:
            w = fold_weight_norm(e["weight_g"], e["weight_v"])      # (the first axis in both layouts: see fold_weight_norm)
        else:
            raise KeyError("layer '{}' has neither weight nor weight_g / weight_v".format(prefix))
        if w.ndim != 3 or "bias" not in e:
            raise ValueError("layer '{}' is not a 1-D convolution with a bias".format(prefix))
        seq.append((prefix, w, np.asarray(e["bias"], dtype=np.float64)))
    if len(seq) < 3:
        raise ValueError("not a MelGAN generator: {} convolutions".format(len(seq)))

    conv = lambda w: conv_kernel(w, dtype)

    out = {"melgan/in/kernel": conv(seq[0][1]), "melgan/in/bias": seq[0][2].astype(dtype)}
    if seq[0][1].shape[2] != 7 or seq[-1][1].shape[2] != 7 or seq[-1][1].shape[0] != 1:
        raise ValueError("not a MelGAN generator: the first and last convolutions must have 7 taps, the last one output channel")
    i, up = 1, 0
    while i < len(seq) - 1:
        prefix, w, b = seq[i]
        if w.shape[2] % 2 or w.shape[0] != 2 * w.shape[1]:
            raise ValueError("layer '{}': expected a ConvTranspose1d [cin, cin / 2, 2r], got {}".format(prefix, w.shape))
        out[f"melgan/up{up}/kernel"] = np.ascontiguousarray(w.transpose(2, 0, 1), dtype=dtype)     # [k, cin, cout]
        out[f"melgan/up{up}/bias"] = b.astype(dtype)
        i += 1
        res = 0
        while i + 3 <= len(seq) - 1 and seq[i][1].shape[2] == 3:
            for leaf, (p, w3, b3) in zip(("conv3", "conv1", "shortcut"), seq[i:i + 3]):
                if w3.shape[2] != (3 if leaf == "conv3" else 1) or w3.shape[0] != w3.shape[1]:
                    raise ValueError("layer '{}': expected the residual block's {} [C, C, {}], got {}".format(
                        p, leaf, 3 if leaf == "conv3" else 1, w3.shape))
                out[f"melgan/up{up}/res{res}/{leaf}/kernel"] = conv(w3)
                out[f"melgan/up{up}/res{res}/{leaf}/bias"] = b3.astype(dtype)
            i += 3
            res += 1
        up += 1
    out["melgan/out/kernel"] = conv(seq[-1][1])
    out["melgan/out/bias"] = seq[-1][2].astype(dtype)
    check_weights(infer_config(out), out)
    return out


def load(path):
    """A generator checkpoint in the public layout (``torch.save`` of its ``state_dict``, bare or under one of the usual keys)
    -> named, folded arrays."""
    # (torch.load as torch defaults it, and whatever the file holds goes on to from_state_dict: HiFi-GAN's loader is the strict one)
    return from_state_dict(vocoder_common.load_state_dict(path, ("state_dict", "generator", "model_g", "netG", "model")))
