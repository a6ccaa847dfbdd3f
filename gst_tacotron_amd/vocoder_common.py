"""What the three vocoders' host modules (melgan.py, hifigan.py, waveglow.py) share: checking named weights against a manifest,
folding weight norm, the project's ``[taps * cin, cout]`` kernel layout, and opening a checkpoint's ``state_dict``.  Each module
keeps these under its own names (``melgan.fold_weight_norm``, ``hifigan.check_weights(cfg, w)``, ...)."""
import numpy as np


def check_weights(manifest, weights):
    """``manifest``: ordered dict name -> shape.  Every name present, every shape the manifest's."""
    for name, shape in manifest.items():
        if name not in weights:
            raise KeyError("missing weight '{}'".format(name))
        got = tuple(np.shape(weights[name]))
        if got != tuple(shape):
            raise ValueError("weight '{}' has shape {}, expected {}".format(name, got, tuple(shape)))


def fold_weight_norm(g, v, transposed=False):
    """``w = g * v / ||v||`` as ``torch.nn.utils.weight_norm(dim=0)`` defines it: the norm runs over every axis but the first, which
    is the output channel of a Conv1d ([cout, cin, k]) and the INPUT channel of a ConvTranspose1d ([cin, cout, k], ``transposed``:
    the same axis, so the flag changes nothing).  float64 in, float64 out."""
    v = np.asarray(v, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64).reshape((v.shape[0],) + (1,) * (v.ndim - 1))
    norm = np.sqrt((v * v).reshape(v.shape[0], -1).sum(axis=1)).reshape(g.shape)
    return g * v / norm


def _np(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t)


def conv_kernel(w, dtype):
    """A Conv1d weight [cout, cin, k] -> the project's [k * cin, cout]"""
    return np.ascontiguousarray(w.transpose(2, 1, 0).reshape(w.shape[2] * w.shape[1], w.shape[0]), dtype=dtype)


def load_state_dict(path, keys=(), weights_only=None, refuse=None):
    """``torch.load`` of a checkpoint on the CPU, unwrapped from the first of ``keys`` under which it holds a dict.  The three
    loaders differ and stay as they are: ``weights_only`` None leaves torch's default (MelGAN, WaveGlow), True is HiFi-GAN's;
    ``refuse``: the message (formatted with the path) for a file that holds no dict, None to pass it on unchecked (MelGAN)."""
    import torch
    sd = torch.load(path, map_location="cpu", **({} if weights_only is None else {"weights_only": weights_only}))
    for key in keys:
        if isinstance(sd, dict) and key in sd and isinstance(sd[key], dict):
            sd = sd[key]
            break
    if refuse is not None and not isinstance(sd, dict):
        raise ValueError(refuse.format(path))
    return sd
