"""The flow vocoder's host side: WaveGlow's configuration (Prenger, Valle & Catanzaro 2019), weight manifest, a seeded synthetic
initialiser and the loader for the public checkpoint layout.  The network itself is stated in include/gsttaco.h
(gsttaco_waveglow_config) and runs in csrc/waveglow.hip; nothing here computes it.

Weights are named, plain (weight norm folded) float32 arrays in the project's ``[taps * cin, cout]`` convention:
``waveglow/up/{kernel [win, mel, mel], bias}``, ``waveglow/flow<k>/W [c_k, c_k]``, ``waveglow/flow<k>/{start,end}/{kernel,bias}``,
``waveglow/flow<k>/layer<i>/{in,cond,res_skip}/{kernel,bias}``.

Only ``state_dict``s are read (a mapping of names to tensors): a checkpoint that pickles the whole model object needs the class that
made it and is not opened here.  No trained WaveGlow checkpoint is at hand, so the loader's layout is NOT verified against one: it is
pinned to torch's own ConvTranspose1d / Conv1d / weight_norm modules on the CPU (tests/test_waveglow_cases.py), as MelGAN's is.
"""
from dataclasses import dataclass

import numpy as np

from . import vocoder_common
from .vocoder_common import _np, conv_kernel, fold_weight_norm

MAX_LAYERS, MAX_FLOWS, MAX_GROUP = 10, 32, 16
_SIZES = ("mel_dim", "hop", "win", "n_group", "n_flows", "n_early_every", "n_early_size", "n_layers", "n_channels")


@dataclass
class WaveGlowConfig:
    mel_dim: int = 80
    hop: int = 256
    win: int = 1024
    n_group: int = 8
    n_flows: int = 12
    n_early_every: int = 4
    n_early_size: int = 2
    n_layers: int = 8
    n_channels: int = 256
    kernel: int = 3

    def flow_channels(self):
        """c_k, k = 0 .. n_flows - 1: n_group less n_early_size for every j in 0 < j <= k with j % n_early_every == 0."""
        return [self.n_group - self.n_early_size * sum(1 for j in range(1, k + 1) if j % self.n_early_every == 0)
                for k in range(self.n_flows)]

    @property
    def n_rem(self):
        return self.flow_channels()[-1]

    @property
    def spect_dim(self):
        return self.mel_dim * self.n_group

    def macs_per_sample(self):
        """Multiply-adds of the WN layers per waveform sample."""
        C = self.n_channels
        return self.n_flows * self.n_layers * ((3 * C + self.spect_dim) * 2 * C + C * 2 * C) / self.n_group

    def check(self):
        """What gsttaco_waveglow_configure refuses on the sizes alone, as a ValueError that names the field."""
        for name in _SIZES:
            if int(getattr(self, name)) < 1:
                raise ValueError("{} must be at least 1".format(name))
        if self.kernel != 3:
            raise ValueError("kernel must be 3")
        if self.n_layers > MAX_LAYERS:
            raise ValueError("n_layers: at most {}".format(MAX_LAYERS))
        if self.n_flows > MAX_FLOWS:
            raise ValueError("n_flows: at most {}".format(MAX_FLOWS))
        if self.n_group > MAX_GROUP:
            raise ValueError("n_group: at most {}".format(MAX_GROUP))
        if self.win % self.hop:
            raise ValueError("win must be a multiple of hop")
        if self.hop % self.n_group:
            raise ValueError("hop must be a multiple of n_group")
        if self.n_group % 2:
            raise ValueError("n_group must be even")
        if self.n_early_size % 2:
            raise ValueError("n_early_size must be even")
        for c in self.flow_channels():
            if c < 2:
                raise ValueError("n_early_size: fewer than 2 channels remain (n_rem < 2)")
            if c % 2:
                raise ValueError("n_early_size: a flow's channel count is odd")
        return self


def from_hp(hp):
    """The configuration of Hyper_Parameters' optional ``Vocoder_WaveGlow`` section, or None without it."""
    sec = hp.get("Vocoder_WaveGlow")
    if sec is None:
        return None
    return WaveGlowConfig(mel_dim=int(hp["Sound"]["Mel_Dim"]), hop=int(hp["Sound"]["Frame_Shift"]),
                          win=int(sec.get("Upsample_Kernel", 4 * int(hp["Sound"]["Frame_Shift"]))), n_group=int(sec.get("Group", 8)),
                          n_flows=int(sec.get("Flows", 12)), n_early_every=int(sec.get("Early_Every", 4)),
                          n_early_size=int(sec.get("Early_Size", 2)), n_layers=int(sec.get("Layers", 8)),
                          n_channels=int(sec.get("Channels", 256))).check()


def manifest(cfg):
    """Ordered dict name -> shape, as gsttaco_waveglow_weight_info reports it."""
    C, S = cfg.n_channels, cfg.spect_dim
    m = {"waveglow/up/kernel": (cfg.win, cfg.mel_dim, cfg.mel_dim), "waveglow/up/bias": (cfg.mel_dim,)}
    for k, c in enumerate(cfg.flow_channels()):
        p = f"waveglow/flow{k}"
        m[p + "/W"] = (c, c)
        m[p + "/start/kernel"], m[p + "/start/bias"] = (c // 2, C), (C,)
        m[p + "/end/kernel"], m[p + "/end/bias"] = (C, c), (c,)
        for i in range(cfg.n_layers):
            q, nrs = f"{p}/layer{i}", (C if i == cfg.n_layers - 1 else 2 * C)
            m[q + "/in/kernel"], m[q + "/in/bias"] = (3 * C, 2 * C), (2 * C,)
            m[q + "/cond/kernel"], m[q + "/cond/bias"] = (S, 2 * C), (2 * C,)
            m[q + "/res_skip/kernel"], m[q + "/res_skip/bias"] = (C, nrs), (nrs,)
    return m


def synthetic_weights(cfg, seed=0, gain_s=0.25):
    """Seeded synthetic weights under which the WN's activations stay O(1) for mels within +-Max_Abs_Mel: normal kernels of variance
    0.5 / (3 C) for ``in``, 0.5 / (2 mel_dim G) for ``cond``, 2 / C for ``res_skip``, 1 / h for ``start``, hop / (mel_dim win) for the
    upsampler, and of standard deviation gain_s / sqrt(0.3 C NL) for ``end`` -- ``gain_s`` moves the log-scales s, and with them how far
    exp(-s) stretches a channel.  Biases ~ N(0, 0.05), N(0, 0.02) for ``end``.  W is the Q of a normal matrix plus N(0, 0.05): well
    conditioned and not orthogonal."""
    rng = np.random.default_rng(seed)
    C, NL = cfg.n_channels, cfg.n_layers
    w = {}
    for name, shape in manifest(cfg).items():
        parts = name.split("/")
        leaf = parts[-2]
        if parts[-1] == "W":
            q, _ = np.linalg.qr(rng.normal(0.0, 1.0, shape))
            a = q + rng.normal(0.0, 0.05, shape)
        elif parts[-1] == "bias":
            a = rng.normal(0.0, 0.02 if leaf == "end" else 0.05, shape)
        elif leaf == "up":
            a = rng.normal(0.0, np.sqrt(cfg.hop / (cfg.mel_dim * cfg.win)), shape)
        elif leaf == "in":
            a = rng.normal(0.0, np.sqrt(0.5 / (3 * C)), shape)
        elif leaf == "cond":
            a = rng.normal(0.0, np.sqrt(0.5 / (2 * cfg.spect_dim)), shape)
        elif leaf == "res_skip":
            a = rng.normal(0.0, np.sqrt(2.0 / C), shape)
        elif leaf == "start":
            a = rng.normal(0.0, np.sqrt(1.0 / shape[0]), shape)
        else:
            a = rng.normal(0.0, gain_s / np.sqrt(0.3 * C * NL), shape)
        w[name] = np.require(np.asarray(a, dtype=np.float32), requirements="C").reshape(shape)
    return w


def check_weights(cfg, weights):
    vocoder_common.check_weights(manifest(cfg), weights)


def infer_config(weights, hop=256):
    """The configuration a set of named arrays was made for.  The upsampler's stride is not in any shape: ``hop`` says it."""
    sh = lambda name: tuple(np.shape(weights[name]))
    win, mel_dim, _ = sh("waveglow/up/kernel")
    chans = []
    while f"waveglow/flow{len(chans)}/W" in weights:
        chans.append(sh(f"waveglow/flow{len(chans)}/W")[0])
    n_layers = 0
    while f"waveglow/flow0/layer{n_layers}/in/kernel" in weights:
        n_layers += 1
    every = next((k for k, c in enumerate(chans) if c != chans[0]), len(chans))
    size = chans[0] - chans[every] if every < len(chans) else 2
    return WaveGlowConfig(mel_dim=mel_dim, hop=int(hop), win=win, n_group=chans[0], n_flows=len(chans), n_early_every=every,
                          n_early_size=size, n_layers=n_layers, n_channels=sh("waveglow/flow0/start/kernel")[1])


def from_state_dict(sd, dtype=np.float32):
    """The project's named, folded arrays of a public-layout WaveGlow ``state_dict``:
    ``upsample.weight`` [mel, mel, win] and ``upsample.bias``; per flow k ``WN.<k>.start``, ``WN.<k>.in_layers.<i>``,
    ``WN.<k>.res_skip_layers.<i>`` as ``weight_g`` / ``weight_v`` / ``bias`` or already folded ``weight``; the conditioning either as ONE
    ``WN.<k>.cond_layer`` of 2 C NL outputs, sliced per layer, or as ``WN.<k>.cond_layers.<i>``; ``WN.<k>.end.weight`` / ``bias``;
    ``convinv.<k>.conv.weight`` [c, c, 1].  Conv1d weights are [cout, cin, taps].  ``dtype``: the arrays' type (float64 keeps the
    folding's full precision)."""
    sd = {k: _np(v) for k, v in sd.items()}

    def folded(prefix):
        if prefix + ".weight" in sd:
            return np.asarray(sd[prefix + ".weight"], dtype=np.float64)
        if prefix + ".weight_g" in sd and prefix + ".weight_v" in sd:
            return fold_weight_norm(sd[prefix + ".weight_g"], sd[prefix + ".weight_v"])
        raise KeyError("layer '{}' has neither weight nor weight_g / weight_v".format(prefix))

    conv = lambda w: conv_kernel(w, dtype)

    def bias(prefix):
        return np.asarray(sd[prefix + ".bias"], dtype=np.float64).astype(dtype)

    up = folded("upsample")
    if up.ndim != 3 or up.shape[0] != up.shape[1]:
        raise ValueError("upsample.weight: expected a ConvTranspose1d [mel, mel, win], got {}".format(up.shape))
    out = {"waveglow/up/kernel": np.ascontiguousarray(up.transpose(2, 0, 1), dtype=dtype), "waveglow/up/bias": bias("upsample")}
    k = 0
    while f"convinv.{k}.conv.weight" in sd:
        p, wn = f"waveglow/flow{k}", f"WN.{k}"
        W = np.asarray(sd[f"convinv.{k}.conv.weight"], dtype=np.float64)
        if W.ndim != 3 or W.shape[0] != W.shape[1] or W.shape[2] != 1:
            raise ValueError("convinv.{}.conv.weight: expected [c, c, 1], got {}".format(k, W.shape))
        out[p + "/W"] = np.ascontiguousarray(W[:, :, 0], dtype=dtype)
        out[p + "/start/kernel"], out[p + "/start/bias"] = conv(folded(wn + ".start")), bias(wn + ".start")
        out[p + "/end/kernel"], out[p + "/end/bias"] = conv(folded(wn + ".end")), bias(wn + ".end")
        C2 = None
        i = 0
        while f"{wn}.in_layers.{i}.bias" in sd:
            q = f"{p}/layer{i}"
            out[q + "/in/kernel"], out[q + "/in/bias"] = conv(folded(f"{wn}.in_layers.{i}")), bias(f"{wn}.in_layers.{i}")
            out[q + "/res_skip/kernel"], out[q + "/res_skip/bias"] = conv(folded(f"{wn}.res_skip_layers.{i}")), bias(f"{wn}.res_skip_layers.{i}")
            C2 = out[q + "/in/bias"].shape[0]
            i += 1
        if i == 0:
            raise KeyError("flow {} has no WN.{}.in_layers".format(k, k))
        if f"{wn}.cond_layer.bias" in sd:           # one conv of 2 C NL outputs: layer i reads outputs [2 C i, 2 C (i + 1))
            cw, cb = conv(folded(wn + ".cond_layer")), bias(wn + ".cond_layer")
            if cw.shape[1] != C2 * i:
                raise ValueError("WN.{}.cond_layer has {} outputs, expected {}".format(k, cw.shape[1], C2 * i))
            for j in range(i):
                out[f"{p}/layer{j}/cond/kernel"] = np.ascontiguousarray(cw[:, C2 * j:C2 * (j + 1)])
                out[f"{p}/layer{j}/cond/bias"] = np.ascontiguousarray(cb[C2 * j:C2 * (j + 1)])
        else:
            for j in range(i):
                out[f"{p}/layer{j}/cond/kernel"] = conv(folded(f"{wn}.cond_layers.{j}"))
                out[f"{p}/layer{j}/cond/bias"] = bias(f"{wn}.cond_layers.{j}")
        k += 1
    if k == 0:
        raise ValueError("not a WaveGlow state_dict: no convinv.0.conv.weight")
    check_weights(infer_config(out), out)
    return out


def load(path):
    """A checkpoint file that holds a WaveGlow ``state_dict`` in the public layout (``torch.save`` of it, bare or under one of the
    usual keys) -> named, folded arrays.  A file that pickles the model object itself is refused: only ``state_dict``s are read."""
    # (torch.load as torch defaults it, as MelGAN's loader; unlike it, a file without a dict is refused here)
    return from_state_dict(vocoder_common.load_state_dict(path, ("state_dict", "model", "waveglow"),
                                                          refuse="'{}' does not hold a state_dict (only state_dicts are read)"))
