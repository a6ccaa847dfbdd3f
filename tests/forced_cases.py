"""Float64 restatement and shared cases of the teacher-forcing tests: tests/test_gpu_forced.py runs them on the GPU,
tests/test_forced_cases.py checks on the CPU that the restatement is the oracle's decoder with one line changed, is well conditioned
in float32 and can see a teacher that is off by one frame.

The reference's decoder loop has two branches under one tf.cond (Taco2.py:183-187): training=False feeds ``decodings[:, -1]`` back
(oracle_np.decoder), training=True consumes ``mels[:, step]`` of ``mels = mels[:, 0:-1:r]`` (Taco2.py:161), i.e. step t reads
``teacher[:, t * r]`` of the [B, Tq, mel] tensor the Feeder builds (Feeder.py:125-139: a zero go frame, the target, padding to a
multiple of r, one more frame).  ``forced_decoder`` is that branch, composed from the oracle's public step functions; every layer
is in inference mode, as everywhere in the library.  S = ceil((Tq - 1) / r) steps.
"""
import collections
import functools

import numpy as np

from gst_tacotron_amd import synthetic, weights
from oracle import oracle_np

TOL = 5e-5              # tests/test_gpu_parity.py's: the project's fp32 bar against the float64 oracle
MIXED_TOL = 2e-2        # tests/test_gpu_parity.py's bar of the bf16 mode


def n_steps(Tq, r):
    return -(-(Tq - 1) // r)


def forced_decoder(hp, w, memory, teacher, dt=np.float64, prenet_masks=None, attn_noise=None, token_lengths=None):
    """oracle_np.decoder (Taco2.py:153-228) with the loop's other branch: step t consumes teacher[:, t * r] (Taco2.py:161,185).
    ``w``: oracle_np.cast_weights(weights, dt); prenet_masks [S, 2, B, size], attn_noise [S, B, T_v].
    Returns pre [B, S*r, mel], stops [B, S], aligns [B, S, T_v]."""
    mel, r = int(hp["Sound"]["Mel_Dim"]), int(hp["Step_Reduction"])
    teacher = np.asarray(teacher, dt)
    B, Tv, _ = memory.shape
    S = n_steps(teacher.shape[1], r)
    pm = oracle_np.process_memory(w, memory)
    sizes = hp["Tacotron2"]["Decoder"]["RNN"]["Size"]
    hs = [np.zeros((B, s), dt) for s in sizes]
    cs = [np.zeros((B, s), dt) for s in sizes]
    is_lsa = hp["Tacotron2"]["Decoder"]["Attention"]["Type"] == "LSA"
    align = np.zeros((B, Tv), dt)
    if not is_lsa:
        align[:, 0] = 1.0                                                    # Steps.py:201-206
    lsa_state = np.zeros((B, Tv), dt)                                        # Layers.py:356
    pre = np.zeros((B, S * r, mel), dt)
    stops = np.zeros((B, S), dt)
    aligns = np.zeros((B, S, Tv), dt)
    for t in range(S):
        frame = teacher[:, t * r]                                            # Taco2.py:185 on mels[:, 0:-1:r]
        masks = None if prenet_masks is None else np.asarray(prenet_masks[t], dt)
        p = oracle_np.prenet(hp, w, frame, masks)
        noise = None if attn_noise is None else np.asarray(attn_noise[t], dt)
        if is_lsa:
            lsa_in = lsa_state
            if token_lengths is not None:
                lsa_in = lsa_state * (np.arange(Tv)[None, :] < np.asarray(token_lengths)[:, None])
            ctx, align, lsa_state = oracle_np.lsa_step(hp, w, p, pm, lsa_in, token_lengths)
        else:
            ctx, align = oracle_np.attention_step(hp, w, p, pm, align, noise, token_lengths)
        x = np.concatenate([p, ctx], -1)
        for i in range(len(sizes)):
            hs[i], cs[i] = oracle_np.lstm_cell(x, hs[i], cs[i], w[f"decoder.lstm{i}.kernel"],
                                               w[f"decoder.lstm{i}.recurrent_kernel"], w[f"decoder.lstm{i}.bias"])
            x = hs[i]
        y = oracle_np.mm(np.concatenate([x, ctx], -1), w["decoder.projection.kernel"]) + w["decoder.projection.bias"]
        pre[:, t * r:(t + 1) * r] = y[:, :mel * r].reshape(B, r, mel)
        stops[:, t] = y[:, mel * r]
        aligns[:, t] = align
    return pre, stops, aligns


def forced_decoder_mixed(*a, **kw):
    """forced_decoder under the oracle's emulation of Use_Mixed_Precision (bf16 GEMM operands; the prenet stays fp32)."""
    prev, oracle_np.MIXED = oracle_np.MIXED, True
    try:
        return forced_decoder(*a, **kw)
    finally:
        oracle_np.MIXED = prev


def behind_go_frame(pre):
    """The teacher whose consumed frames are a free run's own: [zero go frame | pre]  (Tq = 1 + S * r)."""
    return np.concatenate([np.zeros_like(pre[:, :1]), pre], 1)


def durations(align, r, token_lengths=None, mel_lengths=None):
    """NumPy statement of gsttaco_forced_durations: frame f < L_b counts for argmax_{j < n_b} align[b, f // r, j]."""
    align = np.asarray(align)
    B, S, Tv = align.shape
    out = np.zeros((B, Tv), np.int32)
    for b in range(B):
        n = Tv if token_lengths is None else int(token_lengths[b])
        L = S * r if mel_lengths is None else min(int(mel_lengths[b]), S * r)
        for f in range(L):
            out[b, int(np.argmax(align[b, f // r, :n]))] += 1           # (numpy.argmax: the first maximum)
    return out


# ---------------------------------------------------------------------------------------------------- cases
def full_hp(att="SMA", r=2, sizes=None, mixed=False):
    """The reference's decoder sizes (synthetic.config_hp("cfg2"), as tests/test_gpu_parity.py::_full_case); ``att`` "SMA", "BMA" or
    "LSA/filters/kernel"; ``sizes`` = (prenet, lstm, attention) for a smaller decoder."""
    hp = synthetic.config_hp("cfg2")
    dec = hp["Tacotron2"]["Decoder"]
    if att.startswith("LSA"):
        p = att.split("/")
        dec["Attention"] = {"Type": "LSA", "Size": 128, "Conv": {"Filters": int(p[1]), "Kernel_Size": int(p[2])}}
    else:
        dec["Attention"]["Type"] = att
    if sizes is not None:
        dec["Prenet"]["Size"] = [sizes[0], sizes[0]]
        dec["RNN"]["Size"] = [sizes[1], sizes[1]]
        dec["Attention"]["Size"] = sizes[2]
    hp["Step_Reduction"] = r
    if mixed:
        hp["Use_Mixed_Precision"] = True
    return hp


@functools.lru_cache(maxsize=None)
def full_weights(att="SMA", r=2, sizes=None, mixed=False):
    hp = full_hp(att, r, sizes, mixed)
    return hp, weights.synthetic_weights(hp, seed=0)


Shape = collections.namedtuple("Shape", "B Tv r Tq att")
# B, T_v, r, Tq -> S                                   what the row is for
SHAPES = {
    "single_step": Shape(1, 32, 2, 2, "SMA"),          # S = 1
    "ragged_tail": Shape(3, 21, 2, 12, "SMA"),         # S = 6, Tq - 1 = 11 is not a multiple of r
    "rows85": Shape(17, 40, 3, 16, "BMA"),             # S = 5, S * B = 85 rows of the Z0 GEMM: not a multiple of 16
    "two_chunks": Shape(33, 24, 1, 8, "SMA"),          # S = 7, two 32-row chunks
    "three_passes": Shape(2, 300, 2, 9, "BMA"),        # S = 4, three passes of the attention rows
    "lsa": Shape(5, 48, 2, 12, "LSA/32/31"),           # S = 6
}
VARIANT = Shape(5, 48, 2, 12, "SMA")                   # S = 6: the front-end variants, hashed dropout
MASKED = Shape(4, 33, 2, 12, "SMA")
CPU = [Shape(3, 21, r, 1 + 8 * r, att) for att in ("SMA", "BMA") for r in (1, 2, 3)]       # 8 steps each


def make_teacher(rng, B, Tq, mel=80):
    """[B, Tq, mel] clip(N(0, 1.5), -4, 4) like synthetic.make_ref_mels -- frame 0 included: the go frame is used as given."""
    return np.clip(rng.normal(0.0, 1.5, (B, Tq, mel)), -4.0, 4.0).astype(np.float32)


Case = collections.namedtuple("Case", "hp w shape S memory enc gst teacher masks noise token_lengths")


def make_case(shape, seed, sizes=None, mixed=False, token_lengths=None, Tref=12):
    """Inputs of one decode: float64 memory from the oracle's encoder and style-token layer on seeded tokens / reference mels, a
    clipped-normal teacher, injected keep masks and noise."""
    hp, w = full_weights(shape.att, shape.r, sizes, mixed)
    rng = np.random.default_rng(seed)
    tokens, _ = synthetic.make_tokens(rng, shape.B, shape.Tv, lengths=token_lengths)
    mels, ml = synthetic.make_ref_mels(rng, shape.B, Tref)
    S = n_steps(shape.Tq, shape.r)
    prenet = hp["Tacotron2"]["Decoder"]["Prenet"]["Size"]
    masks, noise = synthetic.make_randomness(rng, S, shape.B, shape.Tv, prenet)
    teacher = make_teacher(rng, shape.B, shape.Tq)
    w64 = oracle_np.cast_weights(w, np.float64)
    enc = oracle_np.encoder(hp, w64, tokens, np.float64, token_lengths)
    gst = oracle_np.style_token_layer(hp, w64, mels, ml, np.float64)
    return Case(hp, w, shape, S, oracle_np.gst_concat(enc, gst), enc, gst, teacher, masks, noise, token_lengths)


def reference(case, dt=np.float64, teacher=None, masks=None, noise=None, mixed=False):
    """The forced oracle on a case's inputs (or on another teacher / other randomness)."""
    w = oracle_np.cast_weights(case.w, dt)
    fn = forced_decoder_mixed if mixed else forced_decoder
    return fn(case.hp, w, case.memory.astype(dt), case.teacher if teacher is None else teacher, dt,
              case.masks if masks is None else masks, case.noise if noise is None else noise, case.token_lengths)


def teacher_layout(mel_List, r, mel_dim):
    """Restatement of Feeder.py:103-143 for the mels alone: zero-pad to the longest, prepend the zero go frame, pad to a multiple of
    r, append one more frame."""
    n = max(m.shape[0] for m in mel_List)
    out = np.zeros((len(mel_List), n, mel_dim), np.float32)
    for i, m in enumerate(mel_List):
        out[i, :m.shape[0]] = m
    out = np.hstack([np.zeros((len(mel_List), 1, mel_dim), np.float32), out])
    padded = int(np.ceil(out.shape[1] / r) * r)
    return np.hstack([out, np.zeros((len(mel_List), padded - out.shape[1] + 1, mel_dim), np.float32)])
