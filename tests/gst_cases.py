"""Shapes, size grid and shared float64 references of the style-token (GST) tests: tests/test_gpu_gst.py runs them on the
GPU, tests/test_gst_cases.py checks on the CPU that they are well conditioned and can see what they are meant to see.

The branch under test is the reference-encoder Conv2D stack plus gt_gst_tail_kernel (csrc/gst.hip).  The tail kernel computes
the GRU's input halves TAIL_MAXT = 8 compressed frames per pass, so everything interesting starts above 8 compressed frames:
more than 8 x prod(Strides) reference frames.

Lengths of 0 and lengths beyond the batch width are NOT tested anywhere: the reference gathers GRU step ceil(len/prod)-1
(GST.py:65-68), which is -1 for length 0 and past the sequence for a too-long length -- undefined there, and the oracle's
NumPy indexing would wrap or raise instead of saying what the reference does.
"""
import copy
import functools

import numpy as np

from gst_tacotron_amd import synthetic, weights
from oracle import oracle_np

TAIL_MAXT = 8           # csrc/gst.hip: compressed frames per pass of the tail kernel


class Shape:
    """One batch of reference mels: ``lens`` valid frames per utterance inside ``tref`` frames (+ the prepended frame 0)."""

    def __init__(self, name, tref, lens, seed):
        self.name, self.tref, self.lens, self.seed = name, int(tref), np.asarray(lens, np.int32), int(seed)
        assert self.lens.min() >= 1 and self.lens.max() <= self.tref

    @property
    def B(self):
        return len(self.lens)


# (a) long references at full dimensions: T2 = ceil(1100/64) = 18 compressed frames = passes of 8 + 8 + 2.  The gathered frame is
#     17 (last of the partial pass), 15 (last of pass 2), 16 (first of pass 3), 8 (first of pass 2), 7 (last of pass 1), 9 (inside pass 2).
LONG = Shape("long", 1100, [1100, 1024, 1025, 513, 512, 577], seed=101)
# (a) the default capacity max_ref_frames = 1025: T2 = 16 = exactly two full passes; 33 utterances = a partial 16-row tile of the
#     2-D implicit GEMM and the direct kernel's grid-stride loop (its grid is capped at 8192 workgroups).
CAPACITY = Shape("capacity", 1024, [1024, 1, 64, 65, 1023, 512, 513, 960, 961, 129, 700] + [37 * i + 11 for i in range(22)], seed=102)
# (b) short-length edges: both sides of every compressed-frame boundary of the first two frames, and the shortest / the full length
SHORT = Shape("short", 200, [1, 63, 64, 65, 127, 128, 129, 200], seed=103)
# (e) the small batch that runs between two long ones on the same workspace
SMALL = Shape("small", 70, [70, 33, 64], seed=104)


def _hp(base, mel=None, **gst):
    """``base`` ("tiny" / "cfg2") with the GST sizes given: filters, kernels, strides, rnn, dense, tokens, token_emb, heads, att."""
    hp = synthetic.tiny_hp() if base == "tiny" else synthetic.config_hp("cfg2")
    hp = copy.deepcopy(hp)
    if mel is not None:
        hp["Sound"]["Mel_Dim"] = mel
    ref, st = hp["GST"]["Reference_Encoder"], hp["GST"]["Style_Token"]
    n = len(gst.get("filters", ref["Conv"]["Filters"]))
    ref["Conv"]["Filters"] = list(gst.get("filters", ref["Conv"]["Filters"]))
    ref["Conv"]["Kernel_Size"] = list(gst.get("kernels", [3] * n))
    ref["Conv"]["Strides"] = list(gst.get("strides", [2] * n))
    ref["RNN"]["Size"] = gst.get("rnn", ref["RNN"]["Size"])
    ref["Dense"]["Size"] = gst.get("dense", ref["Dense"]["Size"])
    st["Size"] = gst.get("tokens", st["Size"])
    st["Embedding"]["Size"] = gst.get("token_emb", st["Embedding"]["Size"])
    st["Attention"] = {"Head": gst.get("heads", st["Attention"]["Head"]), "Size": gst.get("att", st["Attention"]["Size"])}
    return hp


class GridCase:
    """One size set.  ``reject``: None when gsttaco_create must accept it (and the GST call must then match the oracle), else the
    text its error must contain -- the name of the offending size."""

    def __init__(self, name, hp, lens, reject=None, wseed=7):
        self.name, self.hp, self.reject, self.wseed = name, hp, reject, wseed
        strides = hp["GST"]["Reference_Encoder"]["Conv"]["Strides"]
        self.stride_prod = int(np.prod(strides))
        self.shape = Shape(name, max(lens), lens, seed=200 + sum(map(ord, name)))
        # every case runs the tail kernel's second pass
        assert -(-self.shape.tref // self.stride_prod) >= TAIL_MAXT + 1, name

    @property
    def mel(self):
        return int(self.hp["Sound"]["Mel_Dim"])


FULL_FILTERS = [32, 32, 64, 64, 128, 128]
# (c) 3 utterances each: the longest gathers compressed frame 9 (second pass), one gathers frame 8 (the first frame of the second
#     pass: its length is 8 x prod + 1), one stays inside the first pass.
GRID = [
    # RNN size 16: 3u/4 = 12 lanes per k-part, KP = 85 k-parts, 4 idle lanes; heads 4, 6 tokens; Cin 1, 4, 4, 8, 8 direct, 16 GEMM
    GridCase("u16_tiny", _hp("tiny"), [600, 513, 130]),
    # RNN 64 (KP = 21, 16 idle lanes); Dense 64 against Attention 256; 8 heads; 33 tokens of a non-default embedding size 48
    GridCase("u64_dense64_att256_heads8_tok33", _hp("tiny", rnn=64, dense=64, att=256, heads=8, tokens=33, token_emb=48), [600, 513, 130]),
    # RNN 128 (KP = 10, 64 idle lanes); one head, one token (softmax over a single score)
    GridCase("u128_heads1_tok1", _hp("tiny", rnn=128, dense=128, att=32, heads=1, tokens=1), [640, 513, 64]),
    # RNN 256 (KP = 5, 64 idle lanes) on the full-size conv stack at 80 mel bins (GRU input 256): 161 536 B of LDS, the largest accepted
    GridCase("u256_mel80_full_filters_tok10", _hp("tiny", mel=80, filters=FULL_FILTERS, rnn=256, dense=128, att=128, heads=4, tokens=10,
                                                  token_emb=256), [600, 513, 130]),
    # ... and with 256 last filters (GRU input 512): 169 728 B against 163 840 B -- refused at create, naming the need
    GridCase("u256_mel80_last_filters256", _hp("tiny", mel=80, filters=[32, 32, 64, 64, 128, 256], rnn=256, dense=128, att=128, heads=4,
                                               tokens=16, token_emb=256), [600, 513, 130], reject="169728 bytes of shared memory"),
    # 12 000 tokens x 4 heads: the scores alone are 192 000 B of shared memory -- refused at create, naming the need
    GridCase("tokens_12000", _hp("tiny", tokens=12000, token_emb=4), [600, 513, 130], reject="shared memory"),
    # layer inputs Cin = 1, 4, 8, 12 take the direct kernel, 16 and 20 the 2-D implicit GEMM (20: a multiple of 4, not of 16); widths 40 .. 2
    GridCase("filters_4_8_12_16_20_32_mel80", _hp("tiny", mel=80, filters=[4, 8, 12, 16, 20, 32], rnn=64, dense=32, att=64, heads=4),
             [600, 513, 130]),
    # Mel_Dim 20 (odd widths down to 1) is not a multiple of 16: create refuses it by name
    GridCase("mel20", _hp("tiny", mel=20), [600, 513, 130], reject="Mel_Dim"),
    # a two-layer stack: stride product 4, GRU input 4 x 16
    GridCase("two_layers", _hp("tiny", filters=[8, 16]), [41, 33, 5]),
    # strides with 1s in them (product 16; widths 40, 20, 20, 10, 10, 5): the stride-1 layers have Cin 8 (direct) and 16 (GEMM)
    GridCase("strides_2_2_1_2_1_2_mel80", _hp("tiny", mel=80, filters=[4, 8, 16, 16, 32, 32], strides=[2, 2, 1, 2, 1, 2]), [150, 129, 17]),
    # kernel sizes 5 and 1: 5 x 5 on the direct kernel (Cin 4) and on the GEMM (Cin 32), 1 x 1 on the GEMM (Cin 16)
    GridCase("kernels_3_5_3_1_3_5_mel80", _hp("tiny", mel=80, filters=[4, 8, 16, 16, 32, 32], kernels=[3, 5, 3, 1, 3, 5]), [600, 513, 130]),
    # what the tail kernel's 16-byte weight loads cannot take: refused at create by name
    GridCase("rnn_6", _hp("tiny", rnn=6), [600, 513, 130], reject="RNN.Size"),
    GridCase("dense_6", _hp("tiny", dense=6), [600, 513, 130], reject="Dense.Size"),
]
GRID_BY_NAME = {c.name: c for c in GRID}


def _frozen(a):
    a = np.array(a, order="C")          # (a copy that keeps 0-d arrays 0-d)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cfg2_weights():
    """(hp, float32 weights) of the full-size model every non-grid GST test uses."""
    hp = synthetic.config_hp("cfg2")
    return hp, {k: _frozen(v) for k, v in weights.synthetic_weights(hp, seed=0).items()}


@functools.lru_cache(maxsize=None)
def grid_weights(name):
    c = GRID_BY_NAME[name]
    return {k: _frozen(v) for k, v in weights.synthetic_weights(c.hp, seed=c.wseed).items()}


@functools.lru_cache(maxsize=None)
def inputs(shape, mel=80):
    """(mels_for_gst [B, tref + 1, mel], lengths [B]) of a Shape, seeded, read-only."""
    mels, lens = synthetic.make_ref_mels(np.random.default_rng(shape.seed), shape.B, shape.tref, mel=mel, lengths=shape.lens)
    return _frozen(mels), _frozen(lens)


def oracle(hp, w, mels, lens, dt=np.float64):
    return oracle_np.style_token_layer(hp, oracle_np.cast_weights(w, dt), np.asarray(mels, dt), lens, dt)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """float64 style embeddings of a Shape at the full dimensions: computed once per process, read-only."""
    hp, w = cfg2_weights()
    return _frozen(oracle(hp, w, *inputs(shape)))


@functools.lru_cache(maxsize=None)
def grid_reference(name):
    c = GRID_BY_NAME[name]
    return _frozen(oracle(c.hp, grid_weights(name), *inputs(c.shape, c.mel)))


def burst_signal(seconds, sample_rate, seed, edge=0.3):
    """Seeded speech-like test signal: noise band-limited to 20-3800 Hz over a white floor 50 dB below it, under an envelope of raised-cosine bursts (0.15-0.5 s, with
    gaps that stay above the trim threshold), with ``edge`` seconds of near silence (-100 dB) at both ends for the trim to remove."""
    rng = np.random.default_rng(seed)
    n, ne = int(seconds * sample_rate), int(edge * sample_rate)
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / sample_rate)
    spec[(f < 20.0) | (f > 3800.0)] = 0.0
    y = np.fft.irfft(spec, n)
    y /= np.abs(y).max()
    env = np.full(n, 0.05)
    pos = ne
    while pos < n - ne:
        ln = int(rng.uniform(0.15, 0.5) * sample_rate)
        ln = min(ln, n - ne - pos)
        env[pos:pos + ln] += rng.uniform(0.3, 0.9) * 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(ln) / max(ln, 1)))
        pos += ln + int(rng.uniform(0.02, 0.1) * sample_rate)
    env[:ne] = env[n - ne:] = 1e-5
    # a white floor 50 dB under the bursts: without it the bins above 3.8 kHz sit AT the front end's -100 dB clip, where the mel value
    # hangs on the last bits of a float32 FFT and the comparison with the float64 oracle would measure that, not the front end
    y = y + 3e-3 * rng.standard_normal(n)
    return _frozen((0.9 * y * env).astype(np.float32))
