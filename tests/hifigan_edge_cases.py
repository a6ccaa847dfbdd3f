"""The HiFi-GAN 16-bit operand forms at the edges of their operand types: the tables and references that
tests/test_hifigan_edge_cases.py admits on the CPU and tests/test_gpu_hifigan_edges.py holds csrc/hifigan.hip to.

The probes make a launch's output the device's rounded operand itself.  With a selector matrix as the kernel and zero biases every
output is one product, gain * q(L(x)), plus exact zeros (``selector_probe``); with a delta as the activation it is amp * q(w)
(``weight_probe``).  The expectation is ``launch_reference`` in FLOAT32 -- the device's own arithmetic: the LeakyReLU is
fl32(x * fl32(slope)) there, x * float64(slope) in the float64 run -- compared with ``==``.  ``edge_entries`` states by hand, from the
formats' definitions, what each table value must become; the CPU test holds ``hifigan.round_operand`` and the float32 restatement to
that before any device sees it.

A product that is float32-subnormal (1.0 times a bfloat16 subnormal) is not part of the contract: ``asserted`` leaves it out, and
the pass with gain / amp 2^10 shows the same operands through a float32-normal product."""
import functools

import numpy as np

import hifigan_half_cases as H
from gst_tacotron_amd import hifigan

PRECISIONS = H.PRECISIONS
_C = hifigan.HiFiGANConfig
# resblock 1, one kernel size 3 at dilation 1, one rate 2.  narrow: the residual convs run at 8 channels (one k block of 32, most of it
# padding); wide: at 64 (two k blocks, the transposed conv four), another wave form
PROBE_CFGS = {
    "narrow": _C(mel_dim=8, initial=16, rates=[2], resblock=1, kernels=[3], dilations=[[1]]),
    "wide": _C(mel_dim=8, initial=128, rates=[2], resblock=1, kernels=[3], dilations=[[1]]),
}
# the launches probed, as indices into ``H.launches``: the input conv (scalar staging, no LeakyReLU), the transposed conv and a
# unit's first conv (vector staging, LeakyReLU; conv1 has no residual)
PROBED = (0, 1, 2)
GAIN = np.float32(2.0 ** 10)          # lifts every 16-bit subnormal operand to a float32-normal, still exact, product
F32_MIN_NORMAL = np.float32(2.0 ** -126)

_f = np.float32
FLT_MAX = np.finfo(np.float32).max
BF16_MAX = np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0]
INF, NAN = _f(np.inf), _f(np.nan)


def _up(v):
    return np.nextafter(_f(v), INF)


def _down(v):
    return np.nextafter(_f(v), -INF)


def leaky_f32(x, slope=0.1):
    """The device's LeakyReLU: x > 0 ? x : fl32(x * fl32(slope))."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, x * _f(slope)).astype(np.float32)


def slope_preimage(target, slope=0.1):
    """A float32 x <= 0 with fl32(x * fl32(slope)) == target (target <= 0), or None where no float32 has that image."""
    target = _f(target)
    if np.isinf(target) or target == 0:
        return -abs(target)
    with np.errstate(over="ignore"):
        x = _f(np.float64(target) / np.float64(_f(slope)))
    lo = x
    with np.errstate(over="ignore"):
        for _ in range(16):
            lo = _up(lo)
        for _ in range(33):
            if np.isfinite(lo) and _f(lo * _f(slope)) == target:
                return lo
            lo = _down(lo)
    return None


# ---------------------------------------------------------------------------------------------------- the table, stated by hand
def positive_edges(precision):
    """[(class, x, the operand x must become)], x > 0 or NaN, from the format's definition alone (not from round_operand)."""
    if precision == "bfloat16":     # 8 significant bits: the ulp at 1 is 2^-7; subnormals are multiples of 2^-133
        one, t_dn, t_up = _f(1.0), _f(1.0 + 2.0 ** -8), _f(1.0 + 3 * 2.0 ** -8)
        return [("tie_down", t_dn, one), ("tie_up", t_up, _f(1.0 + 2.0 ** -6)),
                ("beside_tie", _down(t_dn), one), ("beside_tie", _up(t_dn), _f(1.0 + 2.0 ** -7)),
                ("beside_tie", _down(t_up), _f(1.0 + 2.0 ** -7)), ("beside_tie", _up(t_up), _f(1.0 + 2.0 ** -6)),
                ("largest", BF16_MAX, BF16_MAX), ("overflow", FLT_MAX, INF), ("overflow", INF, INF),
                ("subnormal", _f(2.0 ** -133), _f(2.0 ** -133)), ("tie_to_zero", _f(2.0 ** -134), _f(0.0)),
                ("subnormal_tie", _f(3 * 2.0 ** -134), _f(2.0 ** -132)), ("nan", NAN, NAN), ("zero", _f(0.0), _f(0.0))]
    one, tie = _f(1.0), _f(1.0 + 2.0 ** -11)                # float16: 11 significant bits, the ulp at 1 is 2^-10
    sat = _f(65504.0)
    return [("tie_down", tie, one), ("tie_up", _f(1.0 + 3 * 2.0 ** -11), _f(1.0 + 2.0 ** -9)),
            ("beside_tie", _down(tie), one), ("beside_tie", _up(tie), _f(1.0 + 2.0 ** -10)),
            ("largest", sat, sat), ("saturated", _down(65520.0), sat), ("saturated", _f(65520.0), sat),
            ("saturated", _f(1e6), sat), ("saturated", FLT_MAX, sat), ("saturated", INF, sat),
            ("smallest_normal", _f(2.0 ** -14), _f(2.0 ** -14)),
            ("subnormal", _f(2.0 ** -14 - 2.0 ** -24), _f(2.0 ** -14 - 2.0 ** -24)), ("subnormal", _f(2.0 ** -24), _f(2.0 ** -24)),
            ("tie_to_zero", _f(2.0 ** -25), _f(0.0)), ("subnormal", _up(2.0 ** -25), _f(2.0 ** -24)),
            ("subnormal_tie", _f(3 * 2.0 ** -25), _f(2.0 ** -23)), ("nan", NAN, NAN), ("zero", _f(0.0), _f(0.0))]


# what a negative operand on each edge needs behind a LeakyReLU of slope 0.1: an x whose image under fl32(x * fl32(0.1)) IS the
# edge.  Not every float32 has a preimage (x has the coarser grid above a power of two), and the largest bfloat16 has none below
# FLT_MAX; these classes must keep a negative representative all the same
NEGATIVE_BEHIND_THE_SLOPE = {"bfloat16": ("tie_down", "tie_up", "subnormal", "tie_to_zero", "subnormal_tie", "overflow"),
                             "float16": ("tie_down", "tie_up", "saturated", "subnormal", "tie_to_zero", "subnormal_tie")}


@functools.lru_cache(maxsize=None)
def edge_entries(precision, leaky):
    """[(class, sign, x, want)]: ``want`` is the operand the launch must multiply -- q(x) without a LeakyReLU, q(L(x)) behind one.
    Both signs; behind the LeakyReLU the negative x is the slope's preimage of the negative edge, where one exists."""
    out = []
    for cls, x, want in positive_edges(precision):
        out.append((cls, 1, x, want))
        if cls == "nan":
            continue
        if not leaky:
            out.append((cls, -1, -x, -want))
        elif cls in ("saturated", "overflow") and np.isfinite(x):
            # any x far enough out: the image needs no exact value.  (No finite float32 reaches the bfloat16 overflow through 0.1.)
            if precision == "float16":
                out.append((cls, -1, -_f(10.0) * x if x < 1e30 else -x, -want))
        else:
            pre = slope_preimage(-x)
            if pre is not None:
                out.append((cls, -1, pre, -want))
    return tuple(out)


def randoms(seed, n):
    """n seeded N(0, 1) values, a third each times 2^0, 2^-15 (float16's subnormals) and 2^16 (float16's saturation)."""
    z = np.random.default_rng(seed).normal(0.0, 1.0, n)
    return (z * np.array([1.0, 2.0 ** -15, 2.0 ** 16])[np.arange(n) % 3]).astype(np.float32)


def is_subnormal16(q, precision):
    """q: operands already rounded to ``precision`` -> which are non-zero subnormals of that format"""
    q = np.abs(np.asarray(q, dtype=np.float64))
    return (q > 0) & (q < (2.0 ** -14 if precision == "float16" else 2.0 ** -126))


def asserted(want):
    """Where a probe's expectation is compared: everything but float32-subnormal products (the header says nothing of them)."""
    want = np.asarray(want)
    with np.errstate(invalid="ignore"):
        return ~((want != 0) & (np.abs(want) < F32_MIN_NORMAL))


# ---------------------------------------------------------------------------------------------------- 1. selector probes
FINITE_ROWS = (128, 100, 0, 77)     # frames; a row's table has as many entries as the row has frames
BAD_ROW = 61                        # the row of the entries whose operand is not finite: 0 * inf = NaN reaches neighbours


def selector_weights(cfg, gain=1.0):
    """All zero but: the centre tap of in/kernel maps mel channel c to channel c, taps p < r of up0/kernel the first C / 2 channels to
    themselves, the centre tap of res0/unit0/conv1/kernel is the identity -- times ``gain``."""
    w = {name: np.zeros(shape, dtype=np.float32) for name, shape in hifigan.manifest(cfg).items()}
    g, ch, r = np.float32(gain), cfg.channels(), cfg.rates[0]
    for c in range(cfg.mel_dim):
        w["hifigan/in/kernel"][3 * cfg.mel_dim + c, c] = g
    for p in range(r):
        for c in range(ch[1]):
            w["hifigan/up0/kernel"][p, c, c] = g
    for c in range(ch[1]):
        w["hifigan/up0/res0/unit0/conv1/kernel"][ch[1] + c, c] = g
    return w


def place_selected(l, q):
    """What the selector launch ``l`` makes of the rounded operands q [L, cin] (gain 1): [L * rate_out / rate_in, cout]."""
    L = q.shape[0]
    if l.kind == "in":
        y = np.zeros((L, l.cout), dtype=q.dtype)
        y[:, :l.cin] = q
        return y
    if l.kind == "conv":
        return q.copy()
    y = np.zeros((L * l.r, l.cout), dtype=q.dtype)        # "up": sample o takes tap (o + r / 2) % r of position (o + r / 2) // r
    for o in range(L * l.r):
        i = (o + l.r // 2) // l.r
        if i < L:                                         # (the other tap that reaches o, k + r of position i - 1, is zero)
            y[o] = q[i, :l.cout]
    return y


def _cyclic(table, L, ch):
    """x[t, c] = table[(t + c) % len]: with len <= L every entry visits every channel, so every lane slot and every k block"""
    t, c = np.arange(L)[:, None], np.arange(ch)[None, :]
    return np.ascontiguousarray(table[(t + c) % len(table)])


@functools.lru_cache(maxsize=None)
def selector_probe(config, index, precision, subnormals_only=False):
    """-> dict(l, frames, x, bad_x, want, bad_want, classes).  ``x``: one array per row of FINITE_ROWS, laid out cyclically from the
    row's table (the finite-operand edges, then seeded randoms up to the row's frames); ``bad_x``: the row BAD_ROW of finite randoms
    with the non-finite-operand entries at a few places; ``want`` / ``bad_want``: ``launch_reference`` in float32 on the selector
    weights (gain 1, or GAIN with ``subnormals_only``: the table is then the subnormal operands alone)."""
    cfg = PROBE_CFGS[config]
    gain = GAIN if subnormals_only else np.float32(1.0)
    l = H.launches(cfg, selector_weights(cfg, gain))[index]
    leaky = l.kind != "in"
    entries = edge_entries(precision, leaky)
    fin = [e for e in entries if np.isfinite(e[3])]
    if subnormals_only:
        fin = [e for e in fin if is_subnormal16(e[3], precision)]
    edges = np.array([e[2] for e in fin], dtype=np.float32)
    xs = []
    for b, n in enumerate(FINITE_ROWS):
        L = n * l.rate_in
        if n == 0:
            xs.append(np.zeros((0, l.cin), dtype=np.float32))
            continue
        assert len(edges) < n
        if subnormals_only:         # seeded operands inside the format's subnormal range, both signs
            top = 2.0 ** -14 if precision == "float16" else 2.0 ** -126
            extra = (np.random.default_rng(70 + b).uniform(-1.0, 1.0, n - len(edges)) * top).astype(np.float32)
        else:
            extra = randoms(50 + b, n - len(edges))
        xs.append(_cyclic(np.concatenate([edges, extra]), L, l.cin))
    bad = [e for e in entries if not np.isfinite(e[3])]
    L = BAD_ROW * l.rate_in
    bad_x = np.random.default_rng(90).normal(0.0, 1.0, (L, l.cin)).astype(np.float32)
    spots = []
    for j, e in enumerate(bad):     # far enough apart that finite stretches remain between them
        t, c = (4 + 12 * j) % L, (3 * j + 1) % min(l.cin, l.cout)
        bad_x[t, c] = e[2]
        spots.append((t, c))
    frames = list(FINITE_ROWS)
    want = H.launch_reference(l, {"x": xs}, frames, precision, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        bad_want = H.launch_reference(l, {"x": [bad_x]}, [BAD_ROW], precision, np.float32)[0]
    for a in xs + [bad_x] + want + [bad_want]:
        a.setflags(write=False)
    return dict(l=l, frames=frames, x=xs, bad_x=bad_x, want=want, bad_want=bad_want, entries=fin, bad_entries=bad, spots=spots, gain=gain,
                leaky=leaky)


# ---------------------------------------------------------------------------------------------------- 2. weight probes
@functools.lru_cache(maxsize=None)
def weight_table(precision, subnormals_only=False):
    """The activation table's entries (no LeakyReLU, both signs, the randoms too) that stay finite when a WEIGHT is rounded: no
    saturation there -- float16's conversion of 65520 and above is inf, and the finalize refuses it."""
    vals = np.array([e[2] for e in edge_entries(precision, False)] + list(randoms(60, 150)), dtype=np.float32)
    with np.errstate(over="ignore"):
        keep = np.isfinite(vals.astype(np.float16).astype(np.float32)) if precision == "float16" else np.isfinite(hifigan.round_operand(vals, precision))
    vals = vals[keep & np.isfinite(vals)]
    if subnormals_only:
        top = 2.0 ** -14 if precision == "float16" else 2.0 ** -126
        more = (np.random.default_rng(61).uniform(-1.0, 1.0, 100) * top).astype(np.float32)
        vals = np.concatenate([vals[is_subnormal16(hifigan.round_operand(vals, precision), precision)], more])
    vals.setflags(write=False)
    return vals


def probe_weights(config, precision, subnormals_only=False):
    """Zero biases; the three probed kernels hold the weight table, cyclically over their flat index; every other kernel is zero."""
    cfg = PROBE_CFGS[config]
    table = weight_table(precision, subnormals_only)
    w = {name: np.zeros(shape, dtype=np.float32) for name, shape in hifigan.manifest(cfg).items()}
    for i in PROBED:
        name = H.launches(cfg)[i].name + "/kernel"
        assert w[name].size >= len(table)
        w[name] = np.ascontiguousarray(table[np.arange(w[name].size) % len(table)].reshape(w[name].shape))
    return w


def weight_probe(config, index, precision, subnormals_only=False, weights=None):
    """-> dict(l, frames, x, want).  The activation of a row is ``amp`` (1, or GAIN against the subnormal weights) at position
    (c + 1) * spacing of channel c and 0 elsewhere -- both exact in every form --, spaced so that every output sample is ONE product:
    tap by tap, the kernel's row of that channel across the output channels.  A second, shorter row cuts the pattern off."""
    cfg = PROBE_CFGS[config]
    w = probe_weights(config, precision, subnormals_only) if weights is None else weights
    l = H.launches(cfg, w)[index]
    amp = GAIN if subnormals_only else np.float32(1.0)
    spacing = 2 if l.kind == "up" else l.taps * l.dil
    L = (l.cin + 1) * spacing           # a spacing of room at either end: every tap of every channel lands inside the full row
    n = -(-L // l.rate_in)
    frames = [n, n // 2 + 1, 0]
    xs = []
    for f in frames:
        x = np.zeros((f * l.rate_in, l.cin), dtype=np.float32)
        for c in range(l.cin):
            if (c + 1) * spacing < x.shape[0]:
                x[(c + 1) * spacing, c] = amp
        xs.append(x)
    want = H.launch_reference(l, {"x": xs}, frames, precision, np.float32)
    return dict(l=l, frames=frames, x=xs, want=want, amp=amp, spacing=spacing)


def place_weights(l, x, q):
    """What the delta activations x [L, cin] read of the rounded kernel q (the launch's own layout), sample by sample, by the
    contract's index arithmetic and without a product: [L * rate_out / rate_in, cout] (times the delta's height)."""
    L = x.shape[0]
    if l.kind == "up":
        y = np.zeros((L * l.r, l.cout), dtype=np.float32)
        for i, c in zip(*np.nonzero(x)):
            for k in range(2 * l.r):
                o = i * l.r - l.r // 2 + k
                if 0 <= o < L * l.r:
                    y[o] += x[i, c] * q[k, c]
        return y
    y = np.zeros((L, l.cout), dtype=np.float32)
    pad = (l.taps - 1) // 2 * l.dil
    for i, c in zip(*np.nonzero(x)):
        for k in range(l.taps):
            t = i + pad - k * l.dil
            if 0 <= t < L:
                y[t] += x[i, c] * q[k * l.cin + c]
    return y


# ---------------------------------------------------------------------------------------------------- 4. the regimes of the real kernels
REGIME_CASES = ("tiny", "odd_channels", "halo")


def draw_small(rng, shape):
    """N(0, 1) * 2^-15: |x| < 2^-14 is |z| < 2, and behind the slope every negative one is far inside float16's subnormals"""
    return (rng.normal(0.0, 1.0, shape) * 2.0 ** -15).astype(np.float32)


def draw_loud(rng, shape):
    """N(0, 1) * 2^16: float16 saturates above z = 0.9995, about 16 % of the draws (a negative one is divided by ten first)"""
    return (rng.normal(0.0, 1.0, shape) * 2.0 ** 16).astype(np.float32)


REGIMES = {"small": (draw_small, PRECISIONS), "loud": (draw_loud, ("float16",))}
