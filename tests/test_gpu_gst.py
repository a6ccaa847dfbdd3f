"""GPU: the style-token (GST) branch -- the reference-encoder Conv2D stack, gt_gst_tail_kernel (csrc/gst.hip), the fork and join in
enqueue_encoder and gsttaco_gst -- against the float64 oracle at long references and odd sizes.  The cases and their shared float64
references live in tests/gst_cases.py; tests/test_gst_cases.py shows on the CPU that they are well conditioned (float32 against float64
<= TOL / 5) and that a wrong gather frame moves the result by >= 100 x TOL.  Everything goes through the public entry points.

Lengths of 0 or beyond the batch width are not tested: the reference's gather is undefined there (see gst_cases).
"""
import copy

import numpy as np
import pytest

import gst_cases as G
from test_audio import MEL_TOL
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu


def _model(hp, w, B, tref1, Tv=8, **kw):
    from gst_tacotron_amd.model import GST_Tacotron
    m = GST_Tacotron(hyper_parameters=hp, max_batch=B, max_tokens=Tv, max_ref_frames=tref1, **kw)
    m.Restore(weights=w)
    return m


def _gst(m, mels, lens):
    import torch
    out = m.Inference_GST_Step(np.array(mels), np.array(lens))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _err(what, got, ref):
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    per = np.abs(got - ref).reshape(got.shape[0], -1).max(axis=1)
    print(what, "max abs err", float(per.max()), "(worst utterance %d)" % int(per.argmax()), "scale", float(np.abs(ref).max()))
    return float(per.max())


def _sole_context():
    import gc
    gc.collect()            # (the persistent decode launch is taken only while the process has one live context)


# ------------------------------------------------------------------ (a), (b): lengths, full dimensions
@pytest.mark.parametrize("shape", [G.LONG, G.CAPACITY, G.SHORT], ids=lambda s: s.name)
def test_reference_lengths_match_oracle(shape):
    """long: 1100 frames = 18 compressed frames = tail passes of 8 + 8 + 2, the gathered frame on every side of both pass boundaries;
    capacity: the default max_ref_frames = 1025 (two full passes) with 33 ragged utterances; short: both sides of the first two
    compressed-frame boundaries."""
    hp, w = G.cfg2_weights()
    mels, lens = G.inputs(shape)
    m = _model(hp, w, shape.B, shape.tref + 1)
    assert _err("gst " + shape.name, _gst(m, mels, lens), G.reference(shape)) <= TOL


# ------------------------------------------------------------------ (c): sizes
@pytest.mark.parametrize("name", [c.name for c in G.GRID])
def test_size_grid_matches_oracle_or_is_refused_at_create(name):
    """Every size set either is refused by gsttaco_create with a message that names the offending size, or runs and matches the oracle:
    a context that exists never fails inside gsttaco_gst.  Which of the two is pinned per case in gst_cases.GRID."""
    from gst_tacotron_amd import capi
    from gst_tacotron_amd.model import GST_Tacotron
    c = G.GRID_BY_NAME[name]
    try:
        m = GST_Tacotron(hyper_parameters=c.hp, max_batch=c.shape.B, max_tokens=8, max_ref_frames=c.shape.tref + 1)
    except capi.GstTacoError as e:
        print(name, "refused at create:", e)
        assert c.reject is not None, "create refused a size set that it is expected to run: %s" % e
        assert c.reject in str(e)
        return
    assert c.reject is None, "create accepted a size set that it is expected to refuse (%s)" % c.reject
    m.Restore(weights=G.grid_weights(name))
    got = _gst(m, *G.inputs(c.shape, c.mel))            # (raises GstTacoError if the launch refuses what create accepted)
    assert _err("gst grid " + name, got, G.grid_reference(name)) <= TOL


# ------------------------------------------------------------------ (d): fork, join, composition
def test_fork_join_and_composition_at_a_long_reference(monkeypatch):
    """32 utterances x 1024 reference frames beside 32 x 16 tokens: the forked GST branch outlasts the encoder convolutions, so a missing
    or misplaced join reads an unfinished style embedding.  Forked (default) and unforked (GSTTACO_GST_FORK=0) are bitwise the same,
    each is bitwise decode(encode, Inference_GST_Step) + postnet on the same model, and the first two utterances match the oracle."""
    import torch
    from gst_tacotron_amd import synthetic
    from oracle import oracle_np
    B, Tv, Tref, steps = 32, 16, 1024, 4
    hp, w = G.cfg2_weights()
    rng = np.random.default_rng(105)
    tokens, tl = synthetic.make_tokens(rng, B, Tv)
    lens = np.full(B, Tref, np.int32)
    lens[1], lens[5], lens[17] = 577, 513, 64
    mels, ml = synthetic.make_ref_mels(rng, B, Tref, lengths=lens)
    masks, noise = synthetic.make_randomness(rng, steps, B, Tv, [256, 256])
    outs = []
    for fork in (None, "0"):
        monkeypatch.delenv("GSTTACO_GST_FORK", raising=False)
        if fork is not None:
            monkeypatch.setenv("GSTTACO_GST_FORK", fork)
        _sole_context()
        m = _model(hp, w, B, Tref + 1, Tv=Tv)
        runs = []
        for _ in range(2):          # the capture and the replay of the cached graph
            mel, stop, _, align = m.Inference_Step(tokens, tl, None, mels, ml, prenet_masks=masks, attn_noise=noise, steps=steps)
            m.synchronize()
            runs.append((mel.cpu().numpy(), stop.cpu().numpy(), align.cpu().numpy()))
        replay = all(np.array_equal(a, b) for a, b in zip(*runs))
        enc = m.encode(tokens)
        gst = m.Inference_GST_Step(mels, ml)
        pre, stop2, align2 = m.decode(enc, gst, masks, noise, steps=steps)
        mel2 = m.postnet(pre)
        m.synchronize()
        composed = [np.array_equal(a, b.cpu().numpy()) for a, b in zip(runs[0], (mel2, stop2, align2))]
        print("GSTTACO_GST_FORK", fork, ": replay bitwise", replay, "; Inference_Step == composition bitwise (mel, stop, alignment)", composed)
        assert replay and all(composed)
        outs.append(runs[0])
        del m
    same = [np.array_equal(a, b) for a, b in zip(*outs)]
    print("forked == unforked bitwise (mel, stop, alignment)", same)
    assert all(same)
    ref = oracle_np.inference_step(hp, w, tokens[:2], mels[:2], ml[:2], masks[:, :, :2], noise[:, :2], steps=steps, dt=np.float64)
    for what, got, exp in (("mel", outs[0][0], ref[0]), ("stop", outs[0][1], ref[1]), ("alignment", outs[0][2], ref[3])):
        assert _err("forked Inference_Step, utterances 0-1, " + what, got[:2], exp) <= TOL


# ------------------------------------------------------------------ (e), (f), (g): the long batch again
def test_workspace_reuse_between_long_and_short_batches():
    """xs / mx / partial of the tail kernel and the conv workspaces carry nothing from one call into the next."""
    hp, w = G.cfg2_weights()
    long_in, small_in = G.inputs(G.LONG), G.inputs(G.SMALL)
    m = _model(hp, w, G.LONG.B, G.LONG.tref + 1)
    long1 = _gst(m, *long_in)
    small = _gst(m, *small_in)
    long2 = _gst(m, *long_in)
    fresh = _gst(_model(hp, w, G.SMALL.B, G.SMALL.tref + 1), *small_in)
    print("short batch after a long one == fresh model bitwise:", np.array_equal(small, fresh),
          "; long batch again == first time bitwise:", np.array_equal(long1, long2))
    assert _err("gst small after long", small, G.reference(G.SMALL)) <= TOL
    assert np.array_equal(small, fresh)
    assert np.array_equal(long1, long2)


def test_batch_order_permutes_the_embeddings():
    hp, w = G.cfg2_weights()
    mels, lens = G.inputs(G.LONG)
    perm = np.array([3, 0, 5, 1, 4, 2])
    m = _model(hp, w, G.LONG.B, G.LONG.tref + 1)
    got = _gst(m, mels, lens)
    got_p = _gst(m, mels[perm], lens[perm])
    print("permuted batch bitwise equal to the permuted embeddings:", np.array_equal(got_p, got[perm]))
    assert _err("gst permuted batch", got_p, G.reference(G.LONG)[perm]) <= TOL
    assert _err("gst permuted against unpermuted run", got_p, got[perm].astype(np.float64)) <= TOL


def test_mixed_precision_leaves_the_gst_branch_in_fp32():
    """The GST layers have the FP32 weight form only: Use_Mixed_Precision changes nothing in Inference_GST_Step, bitwise."""
    hp, w = G.cfg2_weights()
    mixed = copy.deepcopy(hp)
    mixed["Use_Mixed_Precision"] = True
    mels, lens = G.inputs(G.LONG)
    a = _gst(_model(hp, w, G.LONG.B, G.LONG.tref + 1), mels, lens)
    b = _gst(_model(mixed, w, G.LONG.B, G.LONG.tref + 1), mels, lens)
    print("mixed precision == fp32 bitwise:", np.array_equal(a, b))
    assert _err("gst under mixed precision", b, G.reference(G.LONG)) <= TOL
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ (h): a long wav, end to end
def test_long_wav_to_style_embedding():
    """A 9 s reference (526 frames after the trim = 9 compressed frames, a second pass of one frame) beside a 1.5 s one: the mel front
    end against its oracle, then the GST branch on the mels the GPU produced against the oracle on those same mels."""
    import torch
    from oracle import audio_np
    hp, w = G.cfg2_weights()
    snd = hp["Sound"]
    sigs = [G.burst_signal(9.0, snd["Sample_Rate"], seed=1), G.burst_signal(1.5, snd["Sample_Rate"], seed=2)]
    exp = [audio_np.mel_generate(np.array(y), snd, 60) for y in sigs]
    assert exp[0].shape[0] > 8 * 64 and exp[0].shape[0] < sigs[0].shape[0] // snd["Frame_Shift"]       # a second pass; the trim acted
    m = _model(hp, w, 2, 1025, max_wav_seconds=10.0)
    mels, lens = m.Mel_Generate([np.array(y) for y in sigs], 60)
    torch.cuda.synchronize()
    assert [int(n) for n in lens] == [e.shape[0] for e in exp]
    assert mels.shape[1] == 1 + exp[0].shape[0] and float(mels[:, 0].abs().max()) == 0.0
    for i, e in enumerate(exp):
        assert _err("mel front end, wav %d" % i, mels[i:i + 1, 1:1 + e.shape[0]].cpu().numpy(), e[None]) <= MEL_TOL
    gst = m.Inference_GST_Step(mels, lens)
    torch.cuda.synchronize()
    ref = G.oracle(hp, w, mels.cpu().numpy(), lens.cpu().numpy())
    assert _err("gst on the GPU's mels", gst.cpu().numpy(), ref) <= TOL
