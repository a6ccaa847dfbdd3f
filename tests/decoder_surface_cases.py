"""The size surface of the DECODER -- Sound.Mel_Dim, Step_Reduction, prenet / attention / LSTM sizes -- off the size sets every other GPU
test of the decode loop runs (the shipped decoder with Mel_Dim 80 and r <= 2, or one smaller in every dimension that pad_decoder embeds
in it): tests/test_gpu_decoder_surface.py runs the rows on the GPU, tests/test_decoder_surface_cases.py checks on the CPU that each is
well conditioned, covers what it claims and that create refuses what lies outside the surface.

What is under test is plan_decode (csrc/gsttaco.cpp) and the kernels behind its predicates at numbers they have not met: a projection
pack of 32 .. 81 tiles in the persistent kernels (persist_decode.hip, persist_groups.h, persist_bf16.h: 18 .. 27 before), on and across
the three grid inequalities of gt_persist_decode_supported; the lean input-half and projection kernels beside general recurrent bodies
(an LSTM of 1536 units); the four-kernel front end at full size.  Each row names the branch it exists for (``why``) and the plan fields
it must reach (``plan``), which the GPU test asserts through gsttaco_decode_plan_fields.

Every hp starts from synthetic.tiny_hp(gst=False) for the encoder, postnet and vocoder and overrides only Sound.Mel_Dim, Step_Reduction,
Max_Step (= steps x r) and Tacotron2.Decoder; weights are weights.synthetic_weights(hp, seed=7); inputs come from
np.random.default_rng(11), a fresh generator per (row, shape): tokens, reference mels (GST rows), keep masks in the flat layout
[steps][B x P0 | B x P1] the C-ABI takes (the stacked [steps, 2, B, P] tensor of equal sizes is the same memory), attention noise.
Masked lengths are written out, never drawn.

Tolerances: fp32 rows compare at TOL against the float64 oracle; ADMISSION (CPU): 8 x |float32 oracle - float64 oracle| <= TOL for every
row, shape and output; a row that fails is replaced, never widened.

Mixed precision compares against the bf16-emulating oracle at min(MIXED_TOL, drift / 2), drift = |emulated-mixed oracle - fp32-form
oracle|, and a row is admitted when the emulation's own float64 and float32 evaluations agree within drift / 16, as in
tests/hp_surface_cases.py -- but in the MEAN absolute norm over each output of the decode loop (pre_mel, stop, align), not the maximum.
The rows the persistent bf16 kernel's inequality needs have 48 and 64 utterances behind the full-size decoder: 6 steps round ~10^6
activations to bf16, and an activation that differs between two evaluations in its last bits rounds to the neighbouring bf16 value (0.4 %
of that element) several hundred times; the recurrence carries each flip on.  Measured on the oracle alone (EXPERIMENTS.md): the maxima
of drift and spread are 1.0 .. 12 apart at 64 rows over input seeds 11 .. 14 and still below 16 at TWO rows for three seeds of four, so no
row of the required shape passes drift / 16 in the max norm; the means are 27 .. 257 apart on every mixed row.  A path that rounds no
operand, or the wrong one, moves EVERY element and sits at about the mean drift; a flipped rounding moves few.  So: per loop output the
GPU's mean error is held to min(MIXED_TOL, mean drift / 2); every output, the post-postnet mel included, to the suite's MIXED_TOL in the
max norm (tests/test_gpu_parity.py does the same behind deep stacks); and wherever an output IS conditioned in the max norm (max spread <=
max drift / 16) its max error is held to min(MIXED_TOL, max drift / 2) as well.
"""
import collections
import copy
import functools

import numpy as np

import forced_cases as F
from gst_tacotron_amd import synthetic, weights
from oracle import oracle_np

TOL = 5e-5              # tests/test_gpu_parity.py's: the project's fp32 bar against the float64 oracle
MIXED_TOL = 2e-2        # tests/test_gpu_parity.py's
FLOOR_FACTOR = 8.0
WEIGHT_SEED, INPUT_SEED = 7, 11
TREF = 30               # reference frames of the GST rows
OUTPUTS = ("mel", "stop", "align", "pre_mel")
SHIPPED = dict(prenet=(256, 256), att=128, rnn=(1024, 1024))        # the reference's decoder (Hyper_Parameters.json)
# the persistent kernels' grid (persist_decode.hip: PD_NWG workgroups = PD_UTT chain + projection + PD_HELP helpers + plain)
PD_NWG, PD_UTT, PD_HELP = 256, 32, 64


def mixed_tolerance(drift):
    return min(MIXED_TOL, drift / 2)


def hp_case(mel=80, r=2, att_type="SMA", prenet=(256, 256), att=128, rnn=(1024, 1024), gst=False, max_step=24, mixed=False):
    """synthetic.tiny_hp(gst=False) with Sound.Mel_Dim, Step_Reduction, Max_Step and Tacotron2.Decoder's sizes overridden (and the style
    path switched on for ``gst``).  ``att_type`` "SMA", "BMA" or "LSA" (20 location filters of 9 taps)."""
    hp = copy.deepcopy(synthetic.tiny_hp(att_type, r=r, gst=gst, max_step=max_step))
    hp["Sound"]["Mel_Dim"] = int(mel)
    dec = hp["Tacotron2"]["Decoder"]
    dec["Prenet"]["Size"] = [int(p) for p in prenet]
    dec["RNN"]["Size"] = [int(h) for h in rnn]
    dec["Attention"] = {"Type": att_type, "Size": int(att)}
    if att_type == "LSA":
        dec["Attention"]["Conv"] = {"Filters": 20, "Kernel_Size": 9}
    hp["Use_Mixed_Precision"] = bool(mixed)
    return hp


def pj_tiles(mel, r, P0=256):
    """16-column tiles of the projection pack [r frames, stop | padding to a tile | prenet-0 pre-activations] (csrc/gsttaco.cpp proj_z):
    ``P0`` is the prenet size the kernels run, i.e. the reference's 256 wherever the decoder is padded."""
    return ((mel * r + 1 + 15) // 16 * 16 + P0) // 16


# name      the row's name
# hp        the overrides of hp_case
# shapes    (B, Tv, steps) of every call
# plan      {(B, Tv, steps): {field of gsttaco_decode_plan_fields: value}}: what the GPU test asserts the call's plan is; "persist" says
#           whether the whole loop is ONE persistent launch (decode_counters must agree)
# lengths   {(B, Tv, steps): token_lengths} of the masked runs (row 0 has the full length), or None
# mixed     False; "only": the row IS a Use_Mixed_Precision model (the bf16 persistent kernel's inequality); "also": the fp32 row runs
#           under Use_Mixed_Precision as well.  Either way against the bf16-emulating oracle
# forced    also runs teacher-forced (forced_cases.teacher_layout, forced_cases.forced_decoder)
# why       the host or kernel branch the row exists for
Case = collections.namedtuple("Case", "name hp shapes plan lengths mixed forced why")

_PAD_A = dict(prenet=(240, 112), att=96, rnn=(768, 512))       # smaller in every dimension: zero-padded to the reference's
_PAD_B = dict(prenet=(128, 128), att=64, rnn=(512, 512))
_LEAN_LAUNCH = dict(fused=1, lean_front=1, lean_rec=1, z0=1, lean_x0=1, lean_x1=1, lean_proj=1)      # every lean form of the launch path
_P = dict(persist=1, persist_bf16=0, dec_padded=1, **_LEAN_LAUNCH)

CASES = [
    # ------------------------------------------------------------------------------------ (a) the persistent launch, 32 .. 81 projection tiles
    Case("p80x5_sma_full", dict(mel=80, r=5, att_type="SMA"), [(5, 23, 6), (32, 23, 6), (128, 23, 6)],
         {(5, 23, 6): dict(_P, dec_padded=0, pj_tiles=42), (32, 23, 6): dict(_P, dec_padded=0, pj_tiles=42),
          (128, 23, 6): dict(_P, dec_padded=0, pj_tiles=42)}, None, False, False,
         "r = 5 with 80 mels, full-size weights: 42 projection tiles (27 was the most any test ran); B = 5 one M-tile, B = 32 two (84 "
         "projection workgroups, 76 plain), B = 128 the group kernels at 128 + 84 of 256 workgroups"),
    Case("p80x5_bma_masked", dict(mel=80, r=5, att_type="BMA", **_PAD_A), [(5, 23, 6), (32, 23, 6)],
         {(5, 23, 6): dict(_P, pj_tiles=42), (32, 23, 6): dict(_P, pj_tiles=42)},
         {(5, 23, 6): (23, 9, 17, 2, 22)}, False, False,
         "the same 42 tiles under BMA, zero-padded from 240 / 112 - 96 - 768 / 512; B = 5 also masked with ragged token lengths"),
    Case("p80x5_lsa", dict(mel=80, r=5, att_type="LSA", **_PAD_B), [(5, 37, 6)],
         {(5, 37, 6): dict(persist=1, persist_bf16=0, dec_padded=1, pj_tiles=42)}, None, False, False,
         "42 tiles beside the one-group kernel's LSA chain (T_v <= 128)"),
    Case("p128x5_gst", dict(mel=128, r=5, att_type="SMA", gst=True, **_PAD_A), [(17, 19, 6), (128, 19, 6)],
         {(17, 19, 6): dict(_P, pj_tiles=57), (128, 19, 6): dict(_P, pj_tiles=57)}, None, False, False,
         "57 tiles: B = 17 has 114 projection workgroups and 46 plain; B = 128 fills 242 of the group kernels' 256; Mel_Dim 128 is the "
         "fused front end's step-0 limit (8 prenet-0 weight rows per lane); GST on: the [gst | enc] Value projection rides along"),
    Case("p112x9", dict(mel=112, r=9, att_type="SMA", **_PAD_A), [(32, 17, 6), (96, 17, 6), (128, 17, 6)],
         {(32, 17, 6): dict(_P, pj_tiles=80), (96, 17, 6): dict(_P, pj_tiles=80),
          (128, 17, 6): dict(_P, persist=0, pj_tiles=80)}, None, False, False,
         "80 tiles: B = 32 is 32 + 160 + 64 = 256, NO plain workgroup; B = 96 on the group kernels is 96 + 160 = 256 exactly; B = 128 "
         "(288) is refused the persistent launch and runs the launch path"),
    Case("p128x8", dict(mel=128, r=8, att_type="BMA", **_PAD_B), [(16, 21, 6), (17, 21, 6)],
         {(16, 21, 6): dict(_P, pj_tiles=81), (17, 21, 6): dict(_P, persist=0, pj_tiles=81)}, None, False, False,
         "81 tiles: B = 16 persists with one M-tile (32 + 81 + 64); B = 17 needs 162 projection workgroups of the 160 there are and "
         "runs the launch path with every lean form"),
    Case("p80x3_bf16", dict(mel=80, r=3, att_type="SMA"), [(64, 20, 6)],
         {(64, 20, 6): dict(persist=1, persist_bf16=1, dec_padded=0, pj_tiles=32, z0=1)}, None, "only", False,
         "the bf16 kernel at 2 x 64 + 32 x 4 = 256 exactly: a chain and a helper per utterance and no plain workgroup"),
    Case("p80x4_bf16", dict(mel=80, r=4, att_type="SMA", **_PAD_A), [(48, 20, 6), (64, 20, 6)],
         {(48, 20, 6): dict(persist=1, persist_bf16=1, dec_padded=1, pj_tiles=37, z0=1),
          (64, 20, 6): dict(persist=0, persist_bf16=0, dec_padded=1, pj_tiles=37, z0=1, fused=1, mirror=1)}, None, "only", False,
         "37 tiles under bf16: B = 48 persists (96 + 111), B = 64 (128 + 148 = 276) is refused and runs the launch path on the bf16 "
         "mirrors"),
    # ------------------------------------------------------------------------------------ (b) own sizes: a dimension above the reference's
    Case("rnn1536x1536", dict(mel=16, r=2, att_type="SMA", prenet=(256, 256), att=128, rnn=(1536, 1536)), [(5, 21, 6), (37, 21, 6)],
         {s: dict(persist=0, dec_padded=0, fused=1, lean_front=1, lean_x0=1, lean_x1=0, lean_rec=0, lean_proj=0, fuse12=0)
          for s in ((5, 21, 6), (37, 21, 6))}, None, False, False,
         "gt_lstm_x_supported looks at the k-block count alone: the lean input-half kernel (nkb 24) with H = 1536, beside a general "
         "layer 2, general recurrent bodies in the front launch's workers and the general projection (nkb 104); 37 rows: the "
         "multi-chunk bodies"),
    Case("rnn1024x1536", dict(mel=16, r=2, att_type="BMA", prenet=(256, 256), att=128, rnn=(1024, 1536)), [(5, 21, 6)],
         {(5, 21, 6): dict(persist=0, dec_padded=0, fused=1, lean_x0=1, lean_x1=1, lean_rec=0, lean_proj=0, fuse12=0)}, None, False, True,
         "both input halves lean (nkb 24 and 64, the second with H = 1536), lean_rec 0 (layer 2's recurrent nkb is 96), projection nkb 104"),
    Case("rnn1536x1024", dict(mel=16, r=3, att_type="SMA", prenet=(256, 256), att=128, rnn=(1536, 1024)), [(5, 21, 6)],
         {(5, 21, 6): dict(persist=0, dec_padded=0, fused=1, lean_x0=1, lean_x1=0, lean_rec=0, lean_proj=1, fuse12=0)}, None, "also", False,
         "gt_launch_proj_lean (nkb 72 beside a 64-k-block layer 2) next to GENERAL recurrent bodies: lean_rec == 0 because layer 1's "
         "recurrent nkb is 96"),
    Case("prenet512x256", dict(mel=16, r=2, att_type="SMA", prenet=(512, 256), att=128, rnn=(1024, 1024)), [(5, 21, 6)],
         {(5, 21, 6): dict(persist=0, dec_padded=0, fused=0)}, None, False, False,
         "a first prenet layer above 256: the four-kernel front end and whole LSTM GEMMs at full size, unequal prenet sizes"),
    Case("prenet128_att256", dict(mel=16, r=2, att_type="SMA", prenet=(128, 128), att=256, rnn=(64, 64)), [(5, 21, 6)],
         {(5, 21, 6): dict(persist=0, dec_padded=0, fused=0)}, None, False, False,
         "one dimension below and one above the reference's: not padded; Attention.Size 256 is the one size with a fused-front "
         "instantiation that ok(P1, A, 8) admits only with P1 <= 128 -- and then front_lds_bytes refuses it (the 128 x 260 memory tile)"),
    Case("att144", dict(mel=16, r=2, att_type="BMA", prenet=(32, 32), att=144, rnn=(64, 64)), [(5, 21, 6)],
         {(5, 21, 6): dict(persist=0, dec_padded=0, fused=0)}, None, False, False,
         "attention.hip at a size that is not a power of two (and above the reference's: not padded)"),
    Case("mel144_shipped", dict(mel=144, r=2, att_type="SMA"), [(5, 21, 6)],
         {(5, 21, 6): dict(persist=0, dec_padded=0, fused=0, pj_tiles=35)}, None, False, False,
         "Mel_Dim 144 is 9 prenet-0 weight rows per lane: gt_dec_front_supported refuses it, the SHIPPED decoder runs the four-kernel "
         "front end and loses every lean form and the persistent launch (Mel_Dim 128, the limit, is p128x5_gst / p128x8)"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CALLS = [(c.name, s) for c in CASES for s in c.shapes]
PERSIST_ROWS = [c.name for c in CASES if any(p.get("persist") for p in c.plan.values())]

# What create must refuse, one field at a time, and the text its message must contain
REFUSALS = [
    ("three prenet layers", dict(prenet=(32, 32, 32)), "Prenet.Size"),
    ("one decoder LSTM layer", dict(rnn=(64,)), "Decoder.RNN.Size"),
    ("prenet size 24", dict(prenet=(24, 32)), "Prenet"),
    ("Attention.Size 272", dict(att=272), "Attention.Size"),
    ("Attention.Size 24", dict(att=24), "Attention.Size"),
    ("Step_Reduction 0", dict(r=0), "Step_Reduction"),
    ("Max_Step < Step_Reduction", dict(r=5, max_step=4), "Max_Step"),
]
_TINY_DEC = dict(mel=16, prenet=(32, 32), att=16, rnn=(64, 64))


def refusal_hp(override):
    return hp_case(**{**_TINY_DEC, **override})


def _frozen(a):
    a = np.array(a, order="C")
    a.setflags(write=False)
    return a


def is_mixed_only(name):
    return BY_NAME[name].mixed == "only"


@functools.lru_cache(maxsize=2)         # (a full-size decoder is ~60 MB of float32: the rows are visited one after the other)
def model_of(name, mixed=False):
    """(hp, float32 weights) of a row; ``mixed`` sets Use_Mixed_Precision, the weights are the same."""
    c = BY_NAME[name]
    steps = max(s[2] for s in c.shapes)
    hp = hp_case(mixed=mixed, max_step=steps * c.hp.get("r", 2), **c.hp)
    return hp, {k: _frozen(v) for k, v in weights.synthetic_weights(hp, seed=WEIGHT_SEED).items()}


Inputs = collections.namedtuple("Inputs", "tokens lengths mels mel_lengths masks noise")


@functools.lru_cache(maxsize=None)
def inputs(name, shape):
    """The inputs of one call of a row: tokens [B, Tv] (ragged where the row has lengths for the shape: those are used by the MASKED run
    only), reference mels (GST rows), keep masks [steps, B x P0 + B x P1], noise [steps, B, Tv]."""
    c = BY_NAME[name]
    B, Tv, steps = shape
    hp = hp_case(**c.hp)
    rng = np.random.default_rng(INPUT_SEED)
    tokens, _ = synthetic.make_tokens(rng, B, Tv)
    mels = ml = None
    if hp["GST"]["Use"]:
        mels, ml = synthetic.make_ref_mels(rng, B, TREF, mel=hp["Sound"]["Mel_Dim"], lengths=[TREF - (7 * b) % 19 for b in range(B)])
    P0, P1 = hp["Tacotron2"]["Decoder"]["Prenet"]["Size"]
    masks = (rng.random((steps, B * (P0 + P1))) >= 0.5).astype(np.float32)
    noise = rng.standard_normal((steps, B, Tv)).astype(np.float32)
    tl = None if not c.lengths or shape not in c.lengths else _frozen(np.asarray(c.lengths[shape], np.int32))
    return Inputs(_frozen(tokens), tl, None if mels is None else _frozen(mels), None if ml is None else _frozen(ml), _frozen(masks),
                  _frozen(noise))


def split_masks(hp, masks, B, dt=np.float64):
    """[steps][B x P0 | B x P1] -> per step (m0 [B, P0], m1 [B, P1]): what oracle_np.prenet indexes."""
    P0, P1 = hp["Tacotron2"]["Decoder"]["Prenet"]["Size"]
    return [(np.asarray(m[:B * P0], dt).reshape(B, P0), np.asarray(m[B * P0:], dt).reshape(B, P1)) for m in masks]


def stacked_masks(hp, masks, B):
    """The same memory as the stacked [steps, 2, B, P] tensor (equal prenet sizes only)."""
    P0, P1 = hp["Tacotron2"]["Decoder"]["Prenet"]["Size"]
    assert P0 == P1
    return np.asarray(masks).reshape(len(masks), 2, B, P0)


def run_oracle(hp, w, x, steps, dt=np.float64, masked=False, mixed=False, teacher=None):
    """oracle_np's Inference_Step on one call -- encoder, style path, decoder, postnet -- with the masks in the flat layout; ``teacher``:
    the decoder is forced_cases.forced_decoder.  ``mixed`` emulates bf16 GEMM operands in ``dt`` arithmetic."""
    w = oracle_np.cast_weights(w, dt)
    B = x.tokens.shape[0]
    tl = x.lengths if masked else None
    prev = oracle_np.MIXED, oracle_np.FUSED_PRENET0
    oracle_np.MIXED, oracle_np.FUSED_PRENET0 = bool(mixed), True
    try:
        memory = oracle_np.encoder(hp, w, x.tokens, dt, tl)
        if hp["GST"]["Use"]:
            memory = oracle_np.gst_concat(memory, oracle_np.style_token_layer(hp, w, x.mels, x.mel_lengths, dt))
        masks, noise = split_masks(hp, x.masks, B, dt), np.asarray(x.noise, dt)
        if teacher is not None:
            pre, stop, align = F.forced_decoder(hp, w, memory, teacher, dt, masks, noise, tl)
        else:
            pre, stop, align = oracle_np.decoder(hp, w, memory, dt, masks, noise, steps, token_lengths=tl)
        return {"mel": oracle_np.postnet(hp, w, pre, dt), "stop": stop, "align": align, "pre_mel": pre}
    finally:
        oracle_np.MIXED, oracle_np.FUSED_PRENET0 = prev


def oracle(name, shape, dt=np.float64, masked=False, mixed=False, forced=False):
    hp, w = model_of(name)
    return run_oracle(hp, w, inputs(name, shape), shape[2], dt, masked, mixed, teacher(name, shape) if forced else None)


@functools.lru_cache(maxsize=None)
def teacher(name, shape):
    """The teacher of the forced run in the Feeder's layout (forced_cases.teacher_layout): B target mels of ragged lengths, the longest
    of steps x r - 1 frames, so that the forced decode has ``steps`` steps."""
    B, Tv, steps = shape
    hp = hp_case(**BY_NAME[name].hp)
    mel, r = hp["Sound"]["Mel_Dim"], hp["Step_Reduction"]
    rng = np.random.default_rng(INPUT_SEED + 1)
    n = steps * r - 1
    t = F.teacher_layout([np.clip(rng.normal(0.0, 1.5, (max(1, n - 2 * b), mel)), -4.0, 4.0).astype(np.float32) for b in range(B)], r, mel)
    assert F.n_steps(t.shape[1], r) == steps
    return _frozen(t)


def err(a, b):
    with np.errstate(invalid="ignore"):
        e = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(e.max()) if np.isfinite(e).all() else float("inf")


def errs(a, b):
    return {k: err(a[k], b[k]) for k in OUTPUTS}


def mean_err(a, b):
    with np.errstate(invalid="ignore"):
        e = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(e.mean()) if np.isfinite(e).all() else float("inf")


def mean_errs(a, b):
    return {k: mean_err(a[k], b[k]) for k in OUTPUTS}


Ref = collections.namedtuple("Ref", "ref floor scale")
MixedRef = collections.namedtuple("MixedRef", "ref drift spread drift_max spread_max")
LOOP_OUTPUTS = ("pre_mel", "stop", "align")         # what the decode loop itself emits (the postnet rounds pre_mel to bf16 again)


def max_norm_conditioned(m, k):
    """The emulation pins output ``k`` in the max norm too: no flipped rounding reaches it (mixed_reference)."""
    return m.spread_max[k] <= m.drift_max[k] / 16


@functools.lru_cache(maxsize=None)
def reference(name, shape, masked=False, forced=False):
    """({output: float64 oracle}, {output: float32 floor}, {output: scale}) of one call: computed once per process, read-only."""
    ref = {k: _frozen(v) for k, v in oracle(name, shape, np.float64, masked, forced=forced).items()}
    return Ref(ref, errs(oracle(name, shape, np.float32, masked, forced=forced), ref), {k: float(np.abs(v).max()) for k, v in ref.items()})


@functools.lru_cache(maxsize=None)
def mixed_reference(name, shape):
    """({output: the bf16-emulating oracle in float64}, its drift from the fp32-form oracle per output, the spread between its float64 and
    float32 evaluations -- a flipped rounding INSIDE the reference shows there), both as MEAN absolute differences, and the same two as
    maxima (see the module's docstring: at these sizes the maxima are ill-conditioned, the means are not)."""
    ref = {k: _frozen(v) for k, v in oracle(name, shape, np.float64, mixed=True).items()}
    fp32_form, emu32 = reference(name, shape).ref, oracle(name, shape, np.float32, mixed=True)
    return MixedRef(ref, mean_errs(ref, fp32_form), mean_errs(emu32, ref), errs(ref, fp32_form), errs(emu32, ref))


# ---------------------------------------------------------------------------------------------------- the persistent grid, by the row's numbers
def grid_numbers(name, shape):
    """(B, MT, pj_tiles, bf16) of a call of a row whose decoder runs at the reference's sizes (shipped or padded)."""
    c = BY_NAME[name]
    hp = hp_case(**c.hp)
    B = shape[0]
    return B, (B + 15) // 16, pj_tiles(hp["Sound"]["Mel_Dim"], hp["Step_Reduction"]), c.mixed == "only"


def grid_inequalities(B, MT, pj, bf16):
    """{inequality: (left-hand side, holds)} -- the one of gt_persist_decode_supported the call falls under (persist_decode.hip)."""
    if bf16:
        return {"2B + pj_tiles*MT <= 256": 2 * B + pj * MT}
    if B <= 32:
        return {"32 + pj_tiles*MT + 64 <= 256": PD_UTT + pj * MT + PD_HELP}
    return {"B + 2*pj_tiles <= 256": B + 2 * pj}
