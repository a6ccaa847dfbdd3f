"""The HiFi-GAN vocoder on 16-bit MFMA operands (gsttaco_hifigan_set_operands): the restatements the tests hold it to.

``half_row`` is ``hifigan_cases.hifigan_row`` with ``hifigan.round_operand`` applied to both operands of every matrix product but
the output conv's: the input (after its LeakyReLU) and the kernel of the input conv, of every transposed conv and of every residual
conv.  Biases, residuals, fusion sums and the output conv are unrounded.

A whole-chain comparison against it cannot be tight: the device rounds an fp32 activation where a float64 run rounds a float64
one; near a tie the two round apart and the difference propagates (``e_h``, the distance of the rounded-operand run from the exact
one, is 1 100 to 50 000 times e32).  A tap dropped at a tile edge is one term in k * C and hides under any chain bar.  So the strict
statement is PER LAUNCH: ``launches`` lists the plan's launches as include/gsttaco.h documents them (gsttaco_hifigan_debug_buffer),
and ``launch_reference`` computes one of them on inputs given row by row -- on the device's own fp32 inputs the rounding is then the
same bits on both sides, and what remains is summation order."""
import functools
from dataclasses import dataclass

import numpy as np

import hifigan_cases as M
from gst_tacotron_amd import hifigan

PRECISIONS = ("bfloat16", "float16")
# A case is admitted only while its rounded-operand run stays this close to the exact one (amplitude 1): seen <= 5.6e-2 and <= 9.2e-3
E_H_MAX = {"bfloat16": 2.0 ** -3, "float16": 2.0 ** -6}
BUF_SUM, BUF_UP, BUF_A, BUF_B = 0, 1, 2, 3
SUM_NONE, SUM_SET, SUM_ADD = 0, 1, 2


# ---------------------------------------------------------------------------------------------------- the chain
def half_row(cfg, w, x, precision):
    """One row alone, operands rounded to ``precision``: x [frames >= 1, mel_dim] -> [frames * hop], in x's dtype."""
    dt = x.dtype
    slope, out_slope = dt.type(cfg.slope), dt.type(cfg.out_slope)
    g = lambda name: np.asarray(w[name], dtype=dt)
    q = lambda a: hifigan.round_operand(a, precision)
    h = M._conv(q(x), q(g("hifigan/in/kernel")), g("hifigan/in/bias"), 7, 1)
    for i, r in enumerate(cfg.rates):
        h = M._transposed(q(M._leaky(h, slope)), q(g(f"hifigan/up{i}/kernel")), g(f"hifigan/up{i}/bias"), r)
        total = None
        for j, (k, dils) in enumerate(zip(cfg.kernels, cfg.dilations)):
            y = h
            for m, d in enumerate(dils):
                p = f"hifigan/up{i}/res{j}/unit{m}/"
                t = M._conv(q(M._leaky(y, slope)), q(g(p + "conv1/kernel")), g(p + "conv1/bias"), k, d)
                if cfg.resblock == 1:
                    t = M._conv(q(M._leaky(t, slope)), q(g(p + "conv2/kernel")), g(p + "conv2/bias"), k, 1)
                y = y + t
            total = y if total is None else total + y
        h = total * dt.type(1.0 / len(cfg.kernels))
    y = M._conv(M._leaky(h, out_slope), g("hifigan/out/kernel"), g("hifigan/out/bias"), 7, 1)
    return np.tanh(y[:, 0])


def half_reference(cfg, weights, mel, frames, precision, dtype=np.float64):
    """``hifigan_cases.hifigan_reference`` with ``half_row``."""
    mel = np.asarray(mel)
    B, T = mel.shape[:2]
    frames = np.minimum(np.asarray(frames), T)
    wav = np.zeros((B, T * cfg.hop), dtype=dtype)
    for b in range(B):
        n = int(frames[b])
        if n >= cfg.min_frames:
            wav[b, :n * cfg.hop] = half_row(cfg, weights, mel[b, :n].astype(dtype), precision)
    return wav


@functools.lru_cache(maxsize=None)
def reference(name, precision, dtype="float64"):
    """The rounded-operand run of a case, computed once and shared; callers leave it unchanged."""
    c = M.CASES[name]
    wav = half_reference(c.cfg, c.weights, c.mel, c.frames_array, precision, dtype=np.dtype(dtype).type)
    wav.setflags(write=False)
    return wav


@functools.lru_cache(maxsize=None)
def e_h(name, precision):
    """max |rounded-operand float64 run - exact float64 run| over the case"""
    return float(np.abs(reference(name, precision) - M.reference(name)[0]).max())


# ---------------------------------------------------------------------------------------------------- one launch
@dataclass
class Launch:
    kind: str               # "in", "up", "conv", "out"
    name: str               # the manifest's name of its weights, without the /kernel or /bias leaf
    cin: int
    cout: int
    taps: int               # "up": 2 r
    dil: int
    r: int                  # "up": the rate
    rate_in: int            # samples per frame of its input and of its output
    rate_out: int
    src: int = -1           # "conv": the buffer read through the LeakyReLU; "up" and "out" read BUF_SUM, "in" the mel
    res: int = -1           # "conv": the buffer added raw, or -1
    dst: int = -1           # the buffer written ("conv" with a sum mode: -1, BUF_SUM alone is written); "out": the wav
    sum: int = SUM_NONE
    scale: float = 1.0      # applied to the fused sum's last write
    slope: float = 0.1
    kernel: object = None   # the launch's weights ([taps * cin, cout]; "up": [2 r, cin, cout]) and bias, where ``launches`` was given them
    bias: object = None


def launches(cfg, weights=None):
    """The launches of gsttaco_hifigan in order, as the header states them under gsttaco_hifigan_debug_buffer; with ``weights`` every
    launch carries its kernel and bias."""
    ch, rate = cfg.channels(), 1
    out = [Launch("in", "hifigan/in", cfg.mel_dim, ch[0], 7, 1, 0, 1, 1, dst=BUF_SUM, slope=cfg.slope)]
    n_k = len(cfg.kernels)
    for i, r in enumerate(cfg.rates):
        c = ch[i + 1]
        out.append(Launch("up", f"hifigan/up{i}", ch[i], c, 2 * r, 1, r, rate, rate * r, src=BUF_SUM, dst=BUF_UP, slope=cfg.slope))
        rate *= r
        for j, (k, dils) in enumerate(zip(cfg.kernels, cfg.dilations)):
            x = BUF_UP
            for m, d in enumerate(dils):
                p = f"hifigan/up{i}/res{j}/unit{m}/"
                last = m == len(dils) - 1
                mode = dict(sum=SUM_SET if j == 0 else SUM_ADD, scale=1.0 / n_k if j == n_k - 1 else 1.0) if last else {}
                if cfg.resblock == 1:
                    out.append(Launch("conv", p + "conv1", c, c, k, d, 0, rate, rate, src=x, dst=BUF_A, slope=cfg.slope))
                    out.append(Launch("conv", p + "conv2", c, c, k, 1, 0, rate, rate, src=BUF_A, res=x, dst=-1 if last else BUF_B,
                                      slope=cfg.slope, **mode))
                    x = BUF_B
                else:
                    dst = BUF_B if x == BUF_A else BUF_A
                    out.append(Launch("conv", p + "conv1", c, c, k, d, 0, rate, rate, src=x, res=x, dst=-1 if last else dst,
                                      slope=cfg.slope, **mode))
                    x = dst
    out.append(Launch("out", "hifigan/out", ch[-1], 1, 7, 1, 0, rate, rate, src=BUF_SUM, slope=cfg.out_slope))
    if weights is not None:
        for l in out:
            l.kernel, l.bias = weights[l.name + "/kernel"], weights[l.name + "/bias"]
    return out


def ws_floats_per_frame(cfg):
    """The widest activation of the chain, floats per mel frame of one row (what a workspace buffer holds per frame)."""
    return max(l.rate_out * M._pad16(l.cout) for l in launches(cfg) if l.kind != "out")


def launch_reference(stage, inputs, lengths, precision, dtype=np.float64):
    """One launch.  ``stage``: a Launch of ``launches(cfg, weights)``; ``inputs``: {"x": rows, "res": rows (a conv with a residual), "sum": rows (SUM_ADD)}, every
    entry a list with one array [lengths[b] * stage.rate_in, channels] per row; ``lengths``: frames per row.  Returns the list of the
    rows' results: [frames * rate_out, cout] -- the activation written, or the fused sum where the launch has a sum mode --, for
    "out" the samples [frames * rate].  A row of 0 frames gives an empty array.  The matrix product's operands are rounded to
    ``precision`` (not the output conv's); everything is computed in ``dtype``."""
    dt = np.dtype(dtype)
    q = lambda a: hifigan.round_operand(a, precision)
    w = np.asarray(stage.kernel, dtype=dt)
    b = np.asarray(stage.bias, dtype=dt)
    slope = dt.type(stage.slope)
    out = []
    for row, n in enumerate(lengths):
        x = np.asarray(inputs["x"][row], dtype=dt)
        assert x.shape == (n * stage.rate_in, stage.cin)
        if n < 1:
            out.append(np.zeros((0,) if stage.kind == "out" else (0, stage.cout), dtype=dt))
        elif stage.kind == "in":
            out.append(M._conv(q(x), q(w), b, 7, 1))
        elif stage.kind == "up":
            out.append(M._transposed(q(M._leaky(x, slope)), q(w), b, stage.r))
        elif stage.kind == "out":
            out.append(np.tanh(M._conv(M._leaky(x, slope), w, b, 7, 1)[:, 0]))
        else:
            v = M._conv(q(M._leaky(x, slope)), q(w), b, stage.taps, stage.dil)
            if stage.res >= 0:
                v = np.asarray(inputs["res"][row], dtype=dt) + v
            if stage.sum == SUM_ADD:
                v = np.asarray(inputs["sum"][row], dtype=dt) + v
            if stage.sum != SUM_NONE:
                v = v * dt.type(stage.scale)
            out.append(v)
    return out


def compose(cfg, weights, x, precision, dtype=np.float64):
    """One row through ``launch_reference``, launch by launch on four buffers as the device runs them: must equal ``half_row``."""
    buf = [None] * 4
    n = x.shape[0]
    wav = None
    for l in launches(cfg, weights):
        ins = {"x": [x if l.kind == "in" else buf[l.src]]}
        if l.res >= 0:
            ins["res"] = [buf[l.res]]
        if l.sum == SUM_ADD:
            ins["sum"] = [buf[BUF_SUM]]
        y = launch_reference(l, ins, [n], precision, dtype)[0]
        if l.kind == "out":
            wav = y
        elif l.sum != SUM_NONE:
            buf[BUF_SUM] = y
        else:
            buf[l.dst] = y
    return wav
