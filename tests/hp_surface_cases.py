"""The hyper-parameter surface of the three modules around the decode loop -- encoder, postnet, CBHG vocoder -- off the two size sets
every other GPU test runs (the shipped Hyper_Parameters.json and synthetic.tiny_hp): tests/test_gpu_hp_surface.py runs the cases on
the GPU, tests/test_hp_surface_cases.py checks on the CPU that each is well conditioned, covers what it claims and that create
refuses what lies outside the surface.

What is under test is the HOST WIRING that turns a model layer into a launch (csrc/gsttaco.cpp: enqueue_encoder / encoder_call,
enqueue_postnet / postnet_call, enqueue_vocoder / vocoder_call, finalize_vocoder, build_lean_bilstm, alloc_workspace, upload_conv's
form gating); the kernels themselves are pinned at their edges by tests/test_gpu_conv_kernels.py.  Each row names the host branch it
exists for (``why``) and the launch forms it must reach (``forms``), which the GPU test asserts through gsttaco_*_variants and the
persistent-BiLSTM counter.

Every hp starts from synthetic.tiny_hp("SMA", r=2, gst=False, max_step=24); weights are weights.synthetic_weights(hp, seed=7);
inputs come from np.random.default_rng(11), a fresh generator per (case, shape): synthetic.make_tokens for the encoder,
clip(N(0, 1.5), -4, 4) mels for the postnet and the vocoder.  Masked lengths are written out, never drawn.

Tolerances: the GPU compares at ``tolerance(floor)`` = max(TOL, 8 x floor) as tests/saturated_cases.py does, where floor is the
float32 oracle against the float64 oracle.  ADMISSION (CPU): 8 x floor <= TOL for every row, so the bound is TOL everywhere; a row
that fails admission is replaced, never widened.  Mixed precision compares against the bf16-emulating oracle at
min(MIXED_TOL, drift / 2), drift = |emulated-mixed oracle - fp32-form oracle|, both in float64: a path that rounds no operand, or the
wrong one, sits at about ``drift`` from the emulation, one flipped bf16 rounding well below it.
"""
import collections
import copy
import functools

import numpy as np

from gst_tacotron_amd import synthetic, weights
from oracle import oracle_np

TOL = 5e-5              # tests/test_gpu_parity.py's: the project's fp32 bar against the float64 oracle
MIXED_TOL = 2e-2        # tests/test_gpu_parity.py's
FLOOR_FACTOR = 8.0
WEIGHT_SEED, INPUT_SEED = 7, 11
# Input seeds that differ from INPUT_SEED, and why.  enc_rnn256_c32 at 65 x 7: with seed 11 the bf16-emulating oracle itself flips a
# rounding between its float64 and float32 evaluations (spread 7.6e-5 against drift 4.6e-4: more than the drift / 16 a mixed case may
# have; 65 x 7 x 512 outputs behind a 256-wide recurrence make a flip likely, seeds 12..23 spread 5e-6..3e-5).  Seed 17 spreads 5.5e-6
# under a drift of 5.3e-4.  Decided by the oracle alone.
INPUT_SEEDS = {("enc_rnn256_c32", (65, 7)): 17}


def tolerance(floor):
    return max(TOL, FLOOR_FACTOR * floor)


def mixed_tolerance(drift):
    return min(MIXED_TOL, drift / 2)


def hp_case(mel=16, spec=33, emb=32, enc_filters=(32, 32, 32), enc_kernels=None, enc_rnn=16, post_filters=(32, 32, 32, 32),
            post_kernels=None, bank=(4, 16), proj_filters=(32, 32), proj_kernels=None, highway=(2, 32), voc_rnn=16, r=2, gst=False,
            max_step=24, mixed=False):
    """synthetic.tiny_hp with the sizes of the three modules overridden.  ``post_filters`` / ``post_kernels`` are Decoder.Conv's (the
    postnet gets one more layer, Mel_Dim filters of 5 taps: Taco2.py:133-134); ``bank`` = (Stack_Count, Filters); ``highway`` =
    (Count, Size).  A vocoder has ``proj_dense`` when proj_filters[-1] != mel and ``highway_in`` when highway[1] != mel."""
    hp = copy.deepcopy(synthetic.tiny_hp("SMA", r=r, gst=gst, max_step=max_step))
    hp["Sound"]["Mel_Dim"], hp["Sound"]["Spectrogram_Dim"] = int(mel), int(spec)
    enc = hp["Tacotron2"]["Encoder"]
    enc["Embedding"]["Size"] = int(emb)
    n = len(enc_filters)
    enc["Conv"] = {**enc["Conv"], "Filters": list(enc_filters), "Kernel_Size": list(enc_kernels or [5] * n), "Strides": [1] * n}
    enc["RNN"]["Size"] = int(enc_rnn)
    dec = hp["Tacotron2"]["Decoder"]
    n = len(post_filters)
    dec["Conv"] = {**dec["Conv"], "Filters": list(post_filters), "Kernel_Size": list(post_kernels or [5] * n), "Strides": [1] * n}
    n = len(proj_filters)
    hp["Vocoder_Taco1"]["CBHG"] = {"Conv_Bank": {"Stack_Count": int(bank[0]), "Filters": int(bank[1])}, "Pool": {"Pool_Size": 2, "Strides": 1},
                                   "Conv1D": {"Filters": list(proj_filters), "Kernel_Size": list(proj_kernels or [3] * n)},
                                   "Highwaynet": {"Count": int(highway[0]), "Size": int(highway[1])},
                                   "RNN": {"Size": int(voc_rnn), "Zoneout": 0.0}}
    hp["Use_Mixed_Precision"] = bool(mixed)
    return hp


# name      the row's name
# module    "encoder" (m.encode against oracle_np.encoder), "postnet" (m.postnet against oracle_np.postnet), "vocoder" (m.vocoder against
#           oracle_np.vocoder_taco1)
# hp        the overrides of hp_case
# shapes    (B, T) of every call: T is Tv for the encoder, Tf for the postnet and the vocoder
# forms     what the GPU test asserts the launches are (see tests/test_gpu_hp_surface.py: "ig" = an implicit-GEMM id on every layer,
#           "wino" = a split Winograd id, "wino_h" = the bounded two-plane fp16 id; "persist" = slabs of the persistent BiLSTM per call)
# lengths   {(B, T): token_lengths} of the masked runs (row 0 has the full length), or None
# mixed     also runs under Use_Mixed_Precision against the bf16-emulating oracle
# why       the host branch the row exists for
Case = collections.namedtuple("Case", "name module hp shapes forms lengths mixed why")

_WINO_LENGTHS = tuple([420] + [420 - 13 * b for b in range(1, 31)] + [1])          # 420, 407, ..., 30, and one utterance of ONE token

CASES = [
    # ------------------------------------------------------------------------------------------------ encoder
    Case("enc_k3_k1_k7_rnn48", "encoder", dict(emb=20, enc_filters=[48, 16, 80], enc_kernels=[3, 1, 7], enc_rnn=48), [(3, 9)],
         {"conv": "ig", "rows_path": False, "persist": {(3, 9): 0}}, {(3, 9): (9, 5, 2)}, True,
         "kernel sizes 3, 1 and 7; Embedding.Size 20 is no multiple of 16 (layer 0 gathers 20-wide rows by token); enqueue_bilstm_steps on the "
         "general skinny body with segments of C/16 = 5 and H/16 = 3 k-blocks: under bf16 a 32-k block straddles [x_t | h]"),
    Case("enc_one_even_rnn128", "encoder", dict(emb=36, enc_filters=[64], enc_kernels=[4], enc_rnn=128), [(17, 3)],
         {"conv": "ig", "rows_path": False, "persist": {(17, 3): 0}}, {(17, 3): (3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1)}, False,
         "one layer; an even kernel pads asymmetrically (same_pad_before: 1 before, 2 after); Tv = 3 is shorter than the kernel; 17 rows "
         "are a ragged 16-row M-tile; H = 128 is no lean / persistent size"),
    Case("enc_rnn256_c32", "encoder", dict(emb=32, enc_filters=[32, 32], enc_kernels=[5, 5], enc_rnn=256), [(2, 7), (65, 7)],
         {"conv": "ig", "rows_path": False, "persist": {(2, 7): 1, (65, 7): 2}}, None, True,
         "build_lean_bilstm and the persistent BiLSTM behind a narrow conv stack: the hoisted GEMM has K = 32, N = 2048 (the split-bf16 "
         "GEMM gate has only met K = 512); 65 rows are two slabs of 64 + 1"),
    Case("enc_eight_layers", "encoder", dict(emb=512, enc_filters=[16, 96, 32, 160, 48, 16, 64, 32], enc_kernels=[5, 2, 9, 5, 1, 6, 3, 5],
                                            enc_rnn=32), [(5, 21)],
         {"conv": "ig", "rows_path": False, "persist": {(5, 21): 0}}, None, False,
         "GSTTACO_MAX_LAYERS layers: w_act's rotation with widths going up and down, sized by max(Embedding.Size, filters) with the "
         "embedding wider than every layer"),
    Case("enc_wino_odd", "encoder", dict(emb=36, enc_filters=[48, 144, 48], enc_kernels=[5, 5, 5], enc_rnn=16), [(32, 420)],
         {"conv": "wino", "rows_path": True, "persist": {(32, 420): 0}}, {(32, 420): _WINO_LENGTHS}, False,
         "encoder_rows_path and the F(2,5) split Winograd at channel counts that are not 512: Cin 36 / 48 / 144 zero-padded to the kernel's "
         "wino_cin, 48 and 144 of 128-column blocks; 105 / 210 / 105 workgroups against enc_wino's gate of 100"),
    # ------------------------------------------------------------------------------------------------ postnet
    Case("post_mixed_kernels", "postnet", dict(mel=32, post_filters=[20, 48, 36, 16], post_kernels=[3, 7, 1, 4]), [(3, 7), (3, 1)],
         {"conv": "ig"}, None, True,
         "no layer but the fixed last one has 5 taps; filter counts that are multiples of 4 only (20, 36); under bf16 the out_bf16 / x_bf16 "
         "hand-over between layers of even widths"),
    Case("post_two_layers", "postnet", dict(mel=16, post_filters=[64], post_kernels=[5]), [(2, 1)],
         {"conv": "ig"}, None, False,
         "post_tanh = 0: no tanh anywhere, so no layer is tanh-fed and none may take the bounded form"),
    Case("post_eight_layers", "postnet", dict(mel=48, post_filters=[8] * 7, post_kernels=[5] * 7), [(2, 11)],
         {"conv": "ig"}, None, False,
         "GSTTACO_MAX_LAYERS layers, tanh behind layers 0..5; w_post's rotation"),
    Case("post_wino_small", "postnet", dict(mel=16, post_filters=[64, 64], post_kernels=[5, 5], max_step=1920), [(32, 1920)],
         {"conv": ["wino", "wino_h", "wino"]}, None, False,
         "240 F(4,5) workgroups, exactly the postnet's gate; layer 1 is tanh-fed and must run the bounded two-plane fp16 form (x_absmax, "
         "wino_split_h_planes), layers 0 and 2 a split Winograd form that is not bounded; Cin 16 zero-padded to wino_cin, 64 / 16 of a "
         "128-column block"),
    # ------------------------------------------------------------------------------------------------ vocoder
    Case("voc_no_dense", "vocoder", dict(mel=32, spec=65, bank=(5, 12), proj_filters=[48, 32], proj_kernels=[3, 3], highway=(3, 32),
                                         voc_rnn=48), [(3, 7)],
         {"conv": "ig", "persist": {(3, 7): 0}}, None, True,
         "neither proj_dense nor highway_in: the residual rides in the last projection's epilogue (a.res = mel_in) and the highway "
         "buffers rotate from there; odd bank width 5 x 12 = 60; H = 48"),
    Case("voc_no_highway_in", "vocoder", dict(mel=48, spec=129, bank=(3, 20), proj_filters=[16], proj_kernels=[5], highway=(1, 48),
                                              voc_rnn=32), [(2, 2)],
         {"conv": "ig", "persist": {(2, 2): 0}}, None, False,
         "proj_dense without highway_in; ONE projection layer, so pool2 and 'last' (no ReLU) fall on the same layer"),
    Case("voc_no_highway", "vocoder", dict(mel=16, spec=257, bank=(16, 8), proj_filters=[32, 32, 16], proj_kernels=[1, 4, 2], highway=(0, 16),
                                           voc_rnn=256), [(2, 19)],
         {"conv": "ig", "persist": {(2, 19): 1}}, None, True,
         "Highwaynet.Count = 0: the highway loop is skipped and the BiLSTM reads the last projection's buffer; three projections with "
         "unit and even kernels; 16 bank kernels with Tf barely above the widest; the lean and persistent BiLSTM in the vocoder"),
    # (Max_Step 40: a vocoder call takes at most Max_Step frames, and 40 frames are what puts Tf above the widest of 32 bank kernels)
    Case("voc_bank32", "vocoder", dict(mel=16, spec=33, bank=(32, 4), proj_filters=[64, 24], proj_kernels=[3, 3], highway=(2, 64),
                                       voc_rnn=16, max_step=40), [(1, 40)],
         {"conv": "ig", "persist": {(1, 40): 0}}, None, False,
         "the maximal Stack_Count; a projection (64) as wide as the highway and wider than Mel_Dim: w_vbuf's sizing; proj_dense AND highway_in"),
    # the fourth combination of the two Dense layers: highway_in without proj_dense (the rows above have the other three)
    Case("voc_highway_in_only", "vocoder", dict(mel=16, spec=33, bank=(2, 8), proj_filters=[24, 16], proj_kernels=[2, 3], highway=(1, 32),
                                                voc_rnn=32), [(2, 5)],
         {"conv": "ig", "persist": {(2, 5): 0}}, None, False,
         "highway_in without proj_dense: the residual in the conv epilogue feeds a Dense, not the highway"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# End to end: Inference_Step(..., with_vocoder=True, return_pre_mel=True), injected masks and noise, 8 steps
E2E = {
    # encoder of enc_k3_k1_k7_rnn48, postnet of post_mixed_kernels, vocoder of voc_no_dense; GST on with tiny_hp's style sizes: the
    # memory is 96 + 16 = 112 wide, no multiple of 32 for the Value projection
    "e2e_odd_gst": dict(hp=dict(mel=32, spec=65, emb=20, enc_filters=[48, 16, 80], enc_kernels=[3, 1, 7], enc_rnn=48,
                                post_filters=[20, 48, 36, 16], post_kernels=[3, 7, 1, 4], bank=(5, 12), proj_filters=[48, 32],
                                proj_kernels=[3, 3], highway=(3, 32), voc_rnn=48, r=3, gst=True), B=3, Tv=9, Tref=70, steps=8),
    # encoder of enc_rnn256_c32, vocoder of voc_no_highway
    "e2e_rnn256_nogst": dict(hp=dict(mel=16, spec=257, emb=32, enc_filters=[32, 32], enc_kernels=[5, 5], enc_rnn=256, bank=(16, 8),
                                     proj_filters=[32, 32, 16], proj_kernels=[1, 4, 2], highway=(0, 16), voc_rnn=256, r=1, gst=False),
                             B=2, Tv=7, Tref=0, steps=8),
}

# What create must refuse, one field at a time, and the text its message must contain
REFUSALS = [
    ("encoder filter 24", dict(enc_filters=[32, 24, 32]), "Conv.Filters"),
    ("Embedding.Size 18", dict(emb=18), "Embedding.Size"),
    ("nine encoder layers", dict(enc_filters=[16] * 9), "Encoder.Conv.Filters"),
    ("postnet filter 6", dict(post_filters=[32, 6, 32]), "Decoder.Conv.Filters"),
    ("Stack_Count 33", dict(bank=(33, 4)), "Stack_Count"),
    ("Highwaynet.Size 24", dict(highway=(2, 24)), "Highwaynet.Size"),
    ("CBHG.RNN.Size 24", dict(voc_rnn=24), "RNN.Size"),
]


def _frozen(a):
    a = np.array(a, order="C")
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def model_of(name, mixed=False):
    """(hp, float32 weights) of a case (``name`` in BY_NAME or E2E); ``mixed`` sets Use_Mixed_Precision, the weights are the same."""
    kw = dict(BY_NAME[name].hp if name in BY_NAME else E2E[name]["hp"])
    hp = hp_case(mixed=mixed, **kw)
    return hp, {k: _frozen(v) for k, v in weights.synthetic_weights(hp, seed=WEIGHT_SEED).items()}


@functools.lru_cache(maxsize=None)
def inputs(name, shape):
    """The input of one call of a case: tokens [B, Tv] int32 for the encoder, mels [B, Tf, Mel_Dim] float32 otherwise."""
    c = BY_NAME[name]
    B, T = shape
    rng = np.random.default_rng(INPUT_SEEDS.get((name, shape), INPUT_SEED))
    if c.module == "encoder":
        return _frozen(synthetic.make_tokens(rng, B, T)[0])
    mel = model_of(name)[0]["Sound"]["Mel_Dim"]
    return _frozen(np.clip(rng.normal(0.0, 1.5, (B, T, mel)), -4.0, 4.0).astype(np.float32))


def lengths_of(name, shape):
    c = BY_NAME[name]
    return None if not c.lengths or shape not in c.lengths else np.asarray(c.lengths[shape], np.int32)


def oracle(name, shape, dt=np.float64, masked=False, mixed=False):
    """The oracle on one call of a case; ``mixed`` emulates bf16 GEMM operands (oracle_np.MIXED) in ``dt`` arithmetic."""
    c = BY_NAME[name]
    hp, w = model_of(name)
    w = oracle_np.cast_weights(w, dt)
    x = inputs(name, shape)
    prev, oracle_np.MIXED = oracle_np.MIXED, bool(mixed)
    try:
        if c.module == "encoder":
            return oracle_np.encoder(hp, w, x, dt, lengths_of(name, shape) if masked else None)
        if c.module == "postnet":
            return oracle_np.postnet(hp, w, np.asarray(x, dt), dt)
        return oracle_np.vocoder_taco1(hp, w, np.asarray(x, dt), dt)
    finally:
        oracle_np.MIXED = prev


def err(a, b):
    with np.errstate(invalid="ignore"):
        e = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(e.max()) if np.isfinite(e).all() else float("inf")


Ref = collections.namedtuple("Ref", "ref floor scale")
MixedRef = collections.namedtuple("MixedRef", "ref drift spread")


@functools.lru_cache(maxsize=None)
def reference(name, shape, masked=False):
    """(float64 oracle output, float32 floor, scale) of one call: computed once per process, read-only."""
    ref = _frozen(oracle(name, shape, np.float64, masked))
    return Ref(ref, err(oracle(name, shape, np.float32, masked), ref), float(np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def mixed_reference(name, shape):
    """(the bf16-emulating oracle in float64, its drift from the fp32-form oracle, the spread between its float64 and float32
    evaluations -- a flipped rounding INSIDE the reference would show there)."""
    ref = _frozen(oracle(name, shape, np.float64, mixed=True))
    return MixedRef(ref, err(ref, reference(name, shape).ref), err(oracle(name, shape, np.float32, mixed=True), ref))


E2E_OUTPUTS = ("mel", "stop", "spectrogram", "align", "pre_mel")
E2eCase = collections.namedtuple("E2eCase", "name hp w tokens mels mel_lengths masks noise steps")


@functools.lru_cache(maxsize=None)
def e2e_case(name):
    e = E2E[name]
    hp, w = model_of(name)
    rng = np.random.default_rng(INPUT_SEED)
    tokens, _ = synthetic.make_tokens(rng, e["B"], e["Tv"])
    mels = ml = None
    if e["Tref"]:
        mels, ml = synthetic.make_ref_mels(rng, e["B"], e["Tref"], mel=hp["Sound"]["Mel_Dim"], lengths=[e["Tref"], e["Tref"] - 5, 33][:e["B"]])
    masks, noise = synthetic.make_randomness(rng, e["steps"], e["B"], e["Tv"], hp["Tacotron2"]["Decoder"]["Prenet"]["Size"])
    return E2eCase(name, hp, w, tokens, mels, ml, masks, noise, e["steps"])


def _e2e_oracle(c, dt):
    mel, stop, spec, align, inter = oracle_np.inference_step(c.hp, c.w, c.tokens, c.mels, c.mel_lengths, c.masks, c.noise, steps=c.steps,
                                                            dt=dt, with_vocoder=True)
    return dict(zip(E2E_OUTPUTS, (mel, stop, spec, align, inter["pre_mel"])))


@functools.lru_cache(maxsize=None)
def e2e_reference(name):
    """({output: float64 oracle}, {output: float32 floor}) of an end-to-end case."""
    c = e2e_case(name)
    ref = {k: _frozen(v) for k, v in _e2e_oracle(c, np.float64).items()}
    f32 = _e2e_oracle(c, np.float32)
    return ref, {k: err(f32[k], ref[k]) for k in E2E_OUTPUTS}
