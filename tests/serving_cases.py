"""One large-capacity context across calls of changing shape: the way the library is served (README's ``serving`` figure,
``Inference_Checked``'s re-runs, ``Inference_GTA`` / ``Evaluate`` between free runs) and the way no other test runs it -- every other GPU
test creates its context at exactly the size of the one call it makes.  tests/test_gpu_serving.py runs the sequences on the GPU,
tests/test_serving_cases.py checks on the CPU that each call is well conditioned and that each sequence holds the transitions it claims.

A SEQUENCE is a model (hp + weights.synthetic_weights(hp, seed=7)), a capacity (max_batch, max_tokens, max_ref_frames), the knobs its
contexts are created under, and an ordered list of CALLS.  What is asked of every call: on the serving context -- created once at the
capacity, having run every call before it -- it gives bit for bit what a fresh context of exactly its own size gives, takes the same
decode plan, and (fp32, injected randomness) stays within TOL of the float64 oracle.  What could break that lives in the host library,
not in any one kernel: pad rows of the blocked activation buffers and their bf16 mirrors that are zeroed at allocation only
(alloc_workspace) while enqueue_decode zeroes per call what the launch path needs; buffers packed by the CALL's sizes inside storage of
the CAPACITY's (w_align's leading dimension steps x Tv, w_noise / w_pm / w_lsa_state B x Tv, w_masks re-laid out for a padded decoder);
plan predicates that read the capacity (w_stash exists only above 32 rows, w_z0g is max(32, B)); one graph cache for every entry point;
masks_lazy, context state set by the last decode.

Models come from what exists: decoder_surface_cases.hp_case (a full-size or zero-padded decoder behind synthetic.tiny_hp's encoder,
postnet and vocoder) for the decode sequences, hp_surface_cases.hp_case for the sequence of the modules around the loop.  Inputs come from
np.random.default_rng(11), a fresh generator per call, drawn as decoder_surface_cases.inputs draws them.  Masked lengths are written
out, never drawn.  Every call has 4 .. 8 decode steps: the hazards are per launch, not per step.

``fp32_launch`` and ``fp32_front4`` are the launch-path sequence under its two knobs: the library reads its knobs once, at create, so
they are two contexts and two entries here.

The ``modules`` model is hp_surface_cases' e2e_odd_gst with the encoder of its enc_wino_odd row (e2e_odd_gst's own encoder has 3, 1 and 7
taps: no Winograd layer, so neither encoder_rows_path nor the F(4,5) gate exists for it), and its capacity is 32 x 960 tokens: the F(4,5)
gate of a 144-filter layer (240 workgroups) opens at 32 x 953.

Tolerances: TOL against the float64 oracle for fp32 calls with injected randomness; ADMISSION (CPU): 8 x |float32 oracle - float64
oracle| <= TOL on every output of such a call, the rule of decoder_surface_cases; a call that fails is replaced, never widened.  Mixed
precision, hashed (``seed=``) and per-utterance (``seeds=``) calls are held bitwise to the fresh context alone: the fresh-context
result is pinned to its own oracle by the tests of those modes, and MIXED_TOL would hide what these sequences look for.

EXCEPTIONS (calls held to TOL against the oracle instead of bitwise to the fresh context, because the difference is a legitimate
capacity-dependent form; DESIGN.md 3.5 names the predicate): none.
"""
import collections
import functools

import numpy as np

import decoder_surface_cases as D
import forced_cases as F
import hp_surface_cases as H
from gst_tacotron_amd import synthetic, weights
from oracle import oracle_np

TOL = D.TOL
FLOOR_FACTOR = D.FLOOR_FACTOR
WEIGHT_SEED, INPUT_SEED = D.WEIGHT_SEED, D.INPUT_SEED
PD_BMAX, PD_TVMAX, PDH_BMAX, PDH_TVMAX, LSA_BMAX, LSA_TVMAX = 128, 256, 64, 192, 32, 128      # persist_decode.hip, persist_bf16.h
BITWISE_EXCEPTIONS = ()         # (sequence, index) of the calls named under EXCEPTIONS above

# entry     "step": Inference_Step; "forced": Inference_Step(teacher_mels=) and Forced_Durations of its alignment; "styled":
#           Inference_GST_Step on the call's reference mels, then Inference_Step(style_embeddings=) on its output; "encode", "gst"
#           (Inference_GST_Step), "vocoder", "postnet": the module alone
# B Tv Tref steps   the call's shape; Tref reference frames (0: none); for "vocoder" / "postnet" ``steps`` is the FRAME count
# rand      "injected" (prenet_masks= / attn_noise=), ("seed", n): hashed throughput mode, ("seeds", first): per-utterance seeds
#           first, first + 1, ...; None for the modules that draw nothing
# lengths   token lengths of a masked call (row 0 has the full length), else None
# vocoder   with_vocoder=True
# plan      the fields of gsttaco_decode_plan_fields the call must reach, on the serving context and on the fresh one; for "encode":
#           rows_path (the embedding lookup launched as rows) and f4 (a layer on the F(4,5) split Winograd kernel)
# why       why the call stands where it stands
Call = collections.namedtuple("Call", "entry B Tv Tref steps rand lengths vocoder plan why")


def call(entry, B, Tv, Tref, steps, rand, plan, why, lengths=None, vocoder=False):
    return Call(entry, B, Tv, Tref, steps, rand, None if lengths is None else tuple(lengths), vocoder, dict(plan), why)


# name      the sequence's name
# kind      "decoder": hp of decoder_surface_cases.hp_case; "modules": of hp_surface_cases.hp_case
# hp        the overrides of that hp_case (Max_Step is set to the longest call's)
# capacity  (max_batch, max_tokens, max_ref_frames) of the serving context
# env       the knobs both the serving and the fresh contexts are created under
# full      the index of the one call meant to equal the capacity in B, Tv and Tref, or None
# shrinks   the dimensions in which some call stands directly behind a larger one
# reaches   the launch forms (FORMS below) the sequence's plans must hold
Sequence = collections.namedtuple("Sequence", "name kind hp capacity env full shrinks reaches calls")

_LEAN = D._LEAN_LAUNCH
_ONE = dict(persist=1, persist_bf16=0, dec_padded=0, mirror=0, **_LEAN)                  # the persistent launch, fp32
_LAUNCH = dict(persist=0, persist_bf16=0, dec_padded=0, mirror=0, **_LEAN)               # the launch path with every lean form
_FRONT4 = dict(persist=0, persist_bf16=0, fused=0)                                       # attention.hip and whole LSTM GEMMs
_BF16 = dict(persist=1, persist_bf16=1, fused=1, z0=1, dec_padded=0)
_LSA_CHAIN = dict(persist=1, persist_bf16=0, fused=1, dec_padded=0)
_LSA_LAUNCH = dict(persist=0, persist_bf16=0, fused=1, dec_padded=0)
_PADDED = dict(_ONE, dec_padded=1)

_L128 = tuple([256] + [256 - (11 * b) % 200 for b in range(1, 128)])        # 256, 245, 234, ..., 57 .. 256: every row its own length
_L17 = (40, 9, 33, 2, 40, 17, 25, 1, 38, 12, 29, 5, 40, 21, 3, 36, 14)
_L40 = tuple([150] + [150 - (7 * b) % 120 for b in range(1, 40)])

_SMA = [
    call("step", 5, 23, 30, 6, "injected", _ONE, "first on the context: 5 rows of 128, 23 tokens of 256 -- the capacity effect alone, nothing stale"),
    call("step", 128, 256, 64, 6, "injected", _ONE, "the capacity itself, masked and ragged: the group kernels, every buffer written to capacity",
         lengths=_L128),
    call("step", 5, 23, 30, 6, "injected", _ONE, "call 0 again: rows 5 .. 15 of every blocked buffer are another utterance's; the one-group kernel "
         "behind the group kernels; w_pctl / w_hpart / w_stash / w_z0g behind a grid of another shape; a graph replay"),
    call("step", 5, 23, 30, 4, "injected", _ONE, "the same at fewer steps: a new leading dimension of w_align, a new graph key"),
    call("step", 33, 129, 17, 6, "injected", _ONE, "a partial second group with one row in its last M-tile, more than 128 tokens (two context chunks)"),
    call("step", 32, 128, 17, 6, ("seed", 4242), _ONE, "hashed: the TV128 instantiation behind one that is not; masks_unused behind injected masks"),
    call("step", 17, 40, 9, 6, ("seeds", 1000), _ONE, "masked with per-utterance seeds: Fill_Randomness writes the tensors the hashed call left alone",
         lengths=_L17),
    call("forced", 5, 23, 30, 6, "injected", dict(_LAUNCH, persist=0), "teacher-forced: the launch path (its zero-fills, w_teach, w_zf) on a context "
         "that has only run persistent launches"),
    call("step", 5, 23, 30, 6, "injected", _ONE, "call 0 a third time: the persistent launch behind launch-path state"),
    call("styled", 3, 23, 30, 6, "injected", _ONE, "styled from Inference_GST_Step's output, with the vocoder: the gst and vocoder segments of "
         "the graph cache behind Inference_Step's", vocoder=True),
]


def _relabel(c, plan, why=None):
    return c._replace(plan=dict(plan), why=why or c.why)


SEQUENCES = [
    Sequence("fp32_sma", "decoder", dict(mel=80, r=2, att_type="SMA", gst=True), (128, 256, 65), {}, 1, ("B", "Tv", "steps", "Tref"),
             ("group", "one_group", "tv128", "forced_launch", "hashed", "seeds", "styled"), _SMA),
    Sequence("fp32_launch", "decoder", dict(mel=80, r=2, att_type="SMA", gst=True), (128, 256, 65), {"GSTTACO_PERSIST_DECODE": "0"}, 1,
             ("B", "Tv", "Tref"), ("launch", "forced_launch"),
             [_relabel(_SMA[0], _LAUNCH, "first on the context, the launch path: its zero-fills sized by this call's MT"),
              _relabel(_SMA[1], _LAUNCH, "the capacity itself: w_h1 / w_h2 / w_c1 / w_c2, w_part and w_arrive written to capacity"),
              _relabel(_SMA[2], _LAUNCH, "call 0 again: the launch path's own zero-fills (w_h1[1], w_h2[1], w_c1, w_c2) and w_arrive behind 128 rows"),
              _relabel(_SMA[4], _LAUNCH, "33 rows: the multi-chunk bodies, a partial second chunk"),
              _relabel(_SMA[8], _LAUNCH, "call 0 a third time, behind three M-tiles"),
              _relabel(_SMA[7], _LAUNCH, "teacher-forced behind free runs that HAVE written w_c1 / w_c2 / w_h1 / w_h2 (on fp32_sma the persistent "
                       "launches before it never touch them): Inference_GTA between free runs on the launch path")]),
    Sequence("fp32_front4", "decoder", dict(mel=80, r=2, att_type="SMA", gst=True), (128, 256, 65), {"GSTTACO_FUSED_FRONT": "0"}, 1,
             ("B", "Tv", "Tref"), ("four_kernel",),
             [_relabel(_SMA[0], _FRONT4, "first on the context: attention.hip, the masks read from w_masks"),
              _relabel(_SMA[1], _FRONT4, "the capacity itself on the four-kernel front end"),
              _relabel(_SMA[2], _FRONT4, "call 0 again: w_p1, w_q, w_xa and w_masks behind 128 rows of 256 tokens")]),
    Sequence("bf16", "decoder", dict(mel=80, r=2, att_type="SMA", mixed=True), (128, 192, 2), {}, None, ("B", "Tv"),
             ("bf16", "mirror_launch"),
             [call("step", 5, 33, 0, 6, "injected", _BF16, "first on the context: the bf16 kernel, 5 rows"),
              call("step", 64, 128, 0, 6, "injected", _BF16, "the bf16 kernel's 64 rows: both ping-pongs of every mirror full"),
              call("step", 5, 33, 0, 6, "injected", _BF16, "call 0 again: rows 5 .. 15 of the mirrors hold stale bf16"),
              call("step", 40, 150, 0, 6, "injected", _BF16, "masked and ragged, more than 128 tokens, a partial third M-tile", lengths=_L40),
              call("step", 65, 60, 0, 6, "injected", dict(persist=0, persist_bf16=0, fused=1, z0=1, mirror=1, dec_padded=0),
                   "above PDH_BMAX: the launch path on the mirrors, P.mirror's zero-fills"),
              call("step", 20, 60, 0, 6, "injected", _BF16, "persistent again: the mirrors of rows 20 .. 31 are the launch path's")]),
    Sequence("lsa", "decoder", dict(mel=80, r=2, att_type="LSA"), (32, 160, 2), {}, None, ("B", "Tv"), ("lsa_chain", "lsa_launch"),
             [call("step", 7, 33, 0, 6, "injected", _LSA_CHAIN, "first on the context: the chain's LSA form"),
              call("step", 20, 128, 0, 6, "injected", _LSA_CHAIN, "the chain's LSA form at its 128 tokens, two M-tiles"),
              call("step", 7, 33, 0, 6, "injected", _LSA_CHAIN, "call 0 again: w_lsa_state and w_pm behind larger ones"),
              call("step", 3, 140, 0, 6, "injected", _LSA_LAUNCH, "above 128 tokens: the launch path, dec_front_lsa.hip, w_lsa_state zeroed per call"),
              call("step", 7, 33, 0, 6, "injected", _LSA_CHAIN, "call 0 a third time, behind the launch path")]),
    Sequence("padded_bma", "decoder", dict(mel=80, r=2, att_type="BMA", **D._PAD_A), (32, 64, 2), {}, 1, ("B", "Tv"), ("one_group",),
             [call("step", 5, 23, 0, 6, "injected", _PADDED, "first on the context: the keep masks re-laid out for the padded prenet"),
              call("step", 32, 64, 0, 6, "injected", _PADDED, "the capacity itself: w_masks written to its end"),
              call("step", 5, 23, 0, 6, "injected", _PADDED, "call 0 again: the re-layout of 5 rows over a 32-row call's w_masks")]),
    Sequence("modules", "modules",
             dict(mel=32, spec=65, emb=36, enc_filters=(48, 144, 48), enc_kernels=(5, 5, 5), enc_rnn=16, post_filters=(20, 48, 36, 16),
                  post_kernels=(3, 7, 1, 4), bank=(5, 12), proj_filters=(48, 32), proj_kernels=(3, 3), highway=(3, 32), voc_rnn=48, r=3, gst=True),
             (32, 960, 130), {}, None, ("B", "Tv", "steps", "Tref"), ("rows_path", "f4", "gather"),
             [call("encode", 32, 960, 0, 0, None, dict(rows_path=1, f4=1), "the longest first, masked: embedding rows in front of layer 0, the "
                   "144-filter layer on F(4,5)", lengths=tuple([960] + [960 - 29 * b for b in range(1, 31)] + [1])),
              call("encode", 3, 9, 0, 0, None, dict(rows_path=0, f4=0), "the token gather and implicit GEMMs behind 30 720 rows of w_act"),
              call("step", 4, 21, 30, 8, "injected", {}, "Inference_Step: the encoder segment is the one `encode` captured its own way",
                   vocoder=True),
              call("encode", 32, 400, 0, 0, None, dict(rows_path=1, f4=0), "exactly 100 F(2,5) workgroups: the rows path without F(4,5)"),
              call("encode", 17, 150, 0, 0, None, dict(rows_path=0, f4=0), "below the rows path's gate, masked",
                   lengths=(150, 3, 77, 149, 1, 60, 150, 12, 101, 8, 33, 150, 2, 90, 45, 120, 7)),
              call("gst", 5, 1, 129, 0, None, {}, "129 reference frames, the capacity's"),
              call("gst", 32, 1, 3, 0, None, {}, "3 frames on 32 rows: w_gconv behind 129 frames"),
              call("gst", 7, 1, 40, 0, None, {}, "40 frames, ragged"),
              call("vocoder", 6, 1, 0, 120, None, {}, "the longest frame count"),
              call("step", 4, 21, 30, 8, "injected", {}, "call 2 again: the vocoder segment behind `vocoder`'s, the encoder's behind `encode`'s",
                   vocoder=True),
              call("vocoder", 2, 1, 0, 7, None, {}, "7 frames behind 120: w_vbank, w_vbuf, the vocoder's BiLSTM state"),
              call("postnet", 8, 1, 0, 120, None, {}, "the longest frame count"),
              call("postnet", 3, 1, 0, 5, None, {}, "5 frames behind 120: w_post's rotation"),
              call("step", 4, 21, 30, 8, "injected", {}, "call 2 a third time", vocoder=True)]),
]
BY_NAME = {s.name: s for s in SEQUENCES}
assert len(BY_NAME) == len(SEQUENCES)
ITEMS = [(s.name, i) for s in SEQUENCES for i in range(len(s.calls))]

# The launch forms a sequence may claim (``reaches``): a predicate over (sequence, call)
FORMS = {
    "group": lambda s, c: c.plan.get("persist") == 1 and not c.plan.get("persist_bf16") and c.B > 32,
    "one_group": lambda s, c: c.plan.get("persist") == 1 and not c.plan.get("persist_bf16") and c.B <= 32,
    # (the chain's TV128 instantiation: at most 128 tokens; the coverage test wants one directly behind a call of more)
    "tv128": lambda s, c: c.plan.get("persist") == 1 and not c.plan.get("persist_bf16") and c.B <= 32 and c.Tv <= 128,
    "bf16": lambda s, c: c.plan.get("persist_bf16") == 1,
    "lsa_chain": lambda s, c: s.hp.get("att_type") == "LSA" and c.plan.get("persist") == 1,
    "lsa_launch": lambda s, c: s.hp.get("att_type") == "LSA" and c.plan.get("persist") == 0 and c.plan.get("fused") == 1,
    "launch": lambda s, c: c.entry == "step" and c.plan.get("persist") == 0 and c.plan.get("fused") == 1 and c.plan.get("lean_front") == 1,
    "forced_launch": lambda s, c: c.entry == "forced" and c.plan.get("persist") == 0 and c.plan.get("fused") == 1,
    "mirror_launch": lambda s, c: c.plan.get("persist") == 0 and c.plan.get("mirror") == 1,
    "four_kernel": lambda s, c: c.plan.get("fused") == 0,
    "hashed": lambda s, c: isinstance(c.rand, tuple) and c.rand[0] == "seed",
    "seeds": lambda s, c: isinstance(c.rand, tuple) and c.rand[0] == "seeds" and c.lengths is not None,
    "styled": lambda s, c: c.entry == "styled" and c.vocoder,
    "rows_path": lambda s, c: c.entry == "encode" and c.plan["rows_path"] == 1 and c.plan["f4"] == 0,
    "f4": lambda s, c: c.entry == "encode" and c.plan["f4"] == 1,
    "gather": lambda s, c: c.entry == "encode" and c.plan["rows_path"] == 0,
}
DECODE_ENTRIES = ("step", "forced", "styled")


def is_mixed(seq):
    return bool(BY_NAME[seq].hp.get("mixed"))


def signature(c):
    """What makes two calls of a sequence the same call: everything but the plan and the reason."""
    return c[:8]


def repeats(seq):
    """[(earlier index, later index)] of the calls of a sequence that are the same call."""
    calls = BY_NAME[seq].calls
    first, out = {}, []
    for i, c in enumerate(calls):
        if signature(c) in first:
            out.append((first[signature(c)], i))
        first.setdefault(signature(c), i)
    return out


def outputs_of(c):
    """The names of what a call returns, in the order the tests report them."""
    if c.entry in DECODE_ENTRIES:
        # (a hashed call: also the keep masks and the noise gsttaco_debug_randomness gives for it -- masks_lazy is context state)
        return (("style",) if c.entry == "styled" else ()) + D.OUTPUTS + (("spectrogram",) if c.vocoder else ()) + \
            (("durations",) if c.entry == "forced" else ()) + (("keep_masks", "noise") if isinstance(c.rand, tuple) and c.rand[0] == "seed" else ())
    return {"encode": ("memory",), "gst": ("style",), "vocoder": ("spectrogram",), "postnet": ("mel",)}[c.entry]


def has_oracle(seq, c):
    """The call is also held to the float64 oracle at TOL: fp32, and no randomness but what the test injects."""
    return not is_mixed(seq) and (c.rand is None or c.rand == "injected")


def fresh_capacity(c):
    """(max_batch, max_tokens, max_ref_frames) of the fresh context of a call: exactly its own size."""
    return c.B, c.Tv, max(c.Tref + 1, 2)


def _frozen(a):
    a = np.array(a, order="C")
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=2)         # (a full-size decoder is ~60 MB of float32: the sequences are visited one after the other)
def model_of(seq):
    """(hp, float32 weights) of a sequence."""
    s = BY_NAME[seq]
    if s.kind == "modules":
        hp = H.hp_case(max_step=max(c.steps * (s.hp["r"] if c.entry in DECODE_ENTRIES else 1) for c in s.calls), **s.hp)
    else:
        hp = D.hp_case(max_step=max(c.steps for c in s.calls) * s.hp["r"], **s.hp)
    return hp, {k: _frozen(v) for k, v in weights.synthetic_weights(hp, seed=WEIGHT_SEED).items()}


def _hp(seq):
    s = BY_NAME[seq]
    return H.hp_case(**s.hp) if s.kind == "modules" else D.hp_case(**s.hp)


def ref_lengths(B, Tref):
    """Reference-mel lengths of a call: row 0 full, the others ragged (decoder_surface_cases.inputs' rule, kept above zero)."""
    return [max(1, Tref - (7 * b) % 19) for b in range(B)]


# tokens lengths mels mel_lengths masks noise: what decoder_surface_cases.run_oracle reads; teacher: the forced call's; x: the module's input
Inputs = collections.namedtuple("Inputs", "tokens lengths mels mel_lengths masks noise teacher x")


@functools.lru_cache(maxsize=None)
def inputs(seq, i):
    """The inputs of call ``i`` of a sequence, from a fresh np.random.default_rng(INPUT_SEED): equal calls have equal inputs."""
    c = BY_NAME[seq].calls[i]
    hp = _hp(seq)
    mel, r = hp["Sound"]["Mel_Dim"], hp["Step_Reduction"]
    rng = np.random.default_rng(INPUT_SEED)
    tl = None if c.lengths is None else _frozen(np.asarray(c.lengths, np.int32))
    if c.entry in ("vocoder", "postnet"):
        x = np.clip(rng.normal(0.0, 1.5, (c.B, c.steps, mel)), -4.0, 4.0).astype(np.float32)
        return Inputs(None, None, None, None, None, None, None, _frozen(x))
    tokens = mels = ml = masks = noise = teacher = None
    if c.entry != "gst":
        tokens = _frozen(synthetic.make_tokens(rng, c.B, c.Tv)[0])
    if c.Tref:
        mels, ml = synthetic.make_ref_mels(rng, c.B, c.Tref, mel=mel, lengths=ref_lengths(c.B, c.Tref))
        mels, ml = _frozen(mels), _frozen(ml)
    if c.entry in DECODE_ENTRIES:
        P0, P1 = hp["Tacotron2"]["Decoder"]["Prenet"]["Size"]
        masks = _frozen((rng.random((c.steps, c.B * (P0 + P1))) >= 0.5).astype(np.float32))
        noise = _frozen(rng.standard_normal((c.steps, c.B, c.Tv)).astype(np.float32))
    if c.entry == "forced":         # (decoder_surface_cases.teacher: ragged targets, the longest of steps x r - 1 frames)
        n = c.steps * r - 1
        teacher = F.teacher_layout([np.clip(rng.normal(0.0, 1.5, (max(1, n - 2 * b), mel)), -4.0, 4.0).astype(np.float32)
                                    for b in range(c.B)], r, mel)
        assert F.n_steps(teacher.shape[1], r) == c.steps
        teacher = _frozen(teacher)
    return Inputs(tokens, tl, mels, ml, masks, noise, teacher, None)


def oracle(seq, i, dt=np.float64):
    """{output: array} of the oracle on one call (has_oracle calls only); "durations" is not among them: the GPU test restates it
    from the alignment it got."""
    s = BY_NAME[seq]
    c = s.calls[i]
    assert has_oracle(seq, c)
    hp, w = model_of(seq)
    x = inputs(seq, i)
    if c.entry in DECODE_ENTRIES:
        out = D.run_oracle(hp, w, x, c.steps, dt, masked=c.lengths is not None, teacher=x.teacher)
        wd = oracle_np.cast_weights(w, dt)
        if c.entry == "styled":
            out["style"] = oracle_np.style_token_layer(hp, wd, x.mels, x.mel_lengths, dt)
        if c.vocoder:
            out["spectrogram"] = oracle_np.vocoder_taco1(hp, wd, out["mel"], dt)
        return out
    wd = oracle_np.cast_weights(w, dt)
    if c.entry == "encode":
        return {"memory": oracle_np.encoder(hp, wd, x.tokens, dt, x.lengths)}
    if c.entry == "gst":
        return {"style": oracle_np.style_token_layer(hp, wd, x.mels, x.mel_lengths, dt)}
    if c.entry == "vocoder":
        return {"spectrogram": oracle_np.vocoder_taco1(hp, wd, np.asarray(x.x, dt), dt)}
    return {"mel": oracle_np.postnet(hp, wd, np.asarray(x.x, dt), dt)}


Ref = collections.namedtuple("Ref", "ref floor scale")


@functools.lru_cache(maxsize=None)
def reference(seq, i):
    """({output: float64 oracle}, {output: float32 floor}, {output: scale}) of one call: computed once per process, read-only.  Equal
    calls of a sequence share one entry."""
    first = {b: a for a, b in repeats(seq)}.get(i, i)
    if first != i:
        return reference(seq, first)
    ref = {k: _frozen(v) for k, v in oracle(seq, i, np.float64).items()}
    f32 = oracle(seq, i, np.float32)
    return Ref(ref, {k: D.err(f32[k], ref[k]) for k in ref}, {k: float(np.abs(v).max()) for k, v in ref.items()})


# ---------------------------------------------------------------------------------------------------- the predicates, by the table's numbers
def expects_persist(seq, c):
    """Whether plan_decode (csrc/gsttaco.cpp) gives a decode call of the sequence the persistent launch, from the table's numbers alone:
    the reference's decoder sizes (shipped or padded), a free run, no knob against it, the form's row and token limits and the grid
    inequality of gt_persist_decode_supported (decoder_surface_cases.grid_inequalities)."""
    s = BY_NAME[seq]
    hp = _hp(seq)
    if s.kind != "decoder" or c.entry == "forced" or s.env.get("GSTTACO_PERSIST_DECODE") == "0" or s.env.get("GSTTACO_FUSED_FRONT") == "0":
        return False
    bf16, lsa = is_mixed(seq), s.hp.get("att_type") == "LSA"
    if bf16 and (lsa or c.B > PDH_BMAX or c.Tv > PDH_TVMAX):
        return False
    if lsa and (c.B > LSA_BMAX or c.Tv > LSA_TVMAX):
        return False
    if c.B > PD_BMAX or c.Tv > PD_TVMAX or (c.B > 32 and s.capacity[0] <= 32):       # (w_stash: allocated above 32 rows of capacity)
        return False
    (_, lhs), = D.grid_inequalities(c.B, (c.B + 15) // 16, D.pj_tiles(hp["Sound"]["Mel_Dim"], hp["Step_Reduction"]), bf16).items()
    return lhs <= D.PD_NWG


def enc_rows_path(cout0, B, Tv):
    """encoder_rows_path (csrc/gsttaco.cpp) for a five-tap layer 0 of ``cout0`` filters: 100 F(2,5) workgroups."""
    return (B * ((Tv + 1) // 2) + 63) // 64 * ((cout0 + 127) // 128) >= 100


def enc_f4(couts, B, Tv):
    """Whether some encoder layer's F(4,5) grid reaches its 240 workgroups (encoder_call, csrc/gsttaco.cpp)."""
    return any((B * ((Tv + 3) // 4) + 63) // 64 * ((n + 127) // 128) >= 240 for n in couts)
