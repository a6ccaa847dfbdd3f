"""GPU: style control -- gt_gst_compose_kernel and the tail kernel's exports (csrc/gst.hip), gsttaco_gst_ex / gsttaco_style_compose /
gsttaco_inference_step_styled -- through the public entry points.  The cases and their float64 restatements live in
tests/style_cases.py; tests/test_style_cases.py shows on the CPU that they are well conditioned (float32 against float64 <= TOL / 5)
and that heads in the wrong order move the results by >= 100 x TOL.
"""
import copy

import numpy as np
import pytest

import gst_cases as G
import style_cases as S
from conftest import load_golden
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu


def _model(hp, w, B, tref1=2, Tv=8, **kw):
    from gst_tacotron_amd.model import GST_Tacotron
    m = GST_Tacotron(hyper_parameters=hp, max_batch=B, max_tokens=Tv, max_ref_frames=tref1, **kw)
    m.Restore(weights=w)
    return m


def _np(*ts):
    import torch
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


def _err(what, got, ref):
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    per = np.abs(got - ref).reshape(got.shape[0], -1).max(axis=1)
    print(what, "max abs err", float(per.max()), "(worst utterance %d)" % int(per.argmax()), "scale", float(np.abs(ref).max()))
    return float(per.max())


def _sole_context():
    import gc
    gc.collect()            # (the persistent decode launch is taken only while the process has one live context)


def _same(what, a, b):
    same = [np.array_equal(x, y) for x, y in zip(a, b)]
    print(what, "bitwise", same)
    return all(same) and len(a) == len(b)


# ------------------------------------------------------------------ 1: compose against float64
@pytest.mark.parametrize("name", S.CASES)
def test_compose_matches_float64(name):
    """The reference's exported (float64) pair gives the reference's embedding, signed unnormalised weights without a query give the
    restatement's, and zero weights without a query give the LayerNorm's beta bitwise."""
    hp, w, shape, _ = S.case(name)
    H, N, A = S.dims(hp)
    p, q = S.exported(name)
    m = _model(hp, w, shape.B)
    got = _np(m.Style_Compose(p.astype(np.float32), q.astype(np.float32)))
    assert _err("compose(p, q) " + name, got, S.reference(name)) <= TOL
    got = _np(m.Style_Compose(np.array(S.signed_weights(name))))          # (a writable copy of the shared, frozen case)
    assert _err("compose(signed weights) " + name, got, S.signed_reference(name)) <= TOL
    got = _np(m.Style_Compose(np.zeros((shape.B, H, N), np.float32)))
    beta = np.broadcast_to(np.asarray(w["gst.mha.ln.beta"], np.float32), (shape.B, A))
    print("compose(0) == beta bitwise:", np.array_equal(got, beta))
    assert got.tobytes() == np.ascontiguousarray(beta).tobytes()


# ------------------------------------------------------------------ 2: export
@pytest.mark.parametrize("name", ["cfg2_short", "sharp_short", "u64_dense64_att256_heads8_tok33"])
def test_export_matches_float64(name):
    hp, w, shape, mel = S.case(name)
    mels, lens = G.inputs(shape, mel)
    p, q = S.exported(name)
    m = _model(hp, w, shape.B, shape.tref + 1)
    plain = _np(m.Inference_GST_Step(np.array(mels), np.array(lens)))
    gst, tw, query = _np(*m.Inference_GST_Step(np.array(mels), np.array(lens), return_attention=True))
    assert _err("token weights " + name, tw, p) <= TOL
    assert _err("query " + name, query, q) <= TOL
    sums = np.abs(tw.astype(np.float64).sum(-1) - 1.0).max()
    print(name, "largest weight", float(tw.max()), "; |sum over tokens - 1| <=", float(sums))
    assert sums <= 1e-6
    assert np.array_equal(gst, plain)
    # the exported pair composes back to the embedding (fp32 rounding: one division by the denominator against one per weight)
    back = _np(m.Style_Compose(tw, query))
    assert _err("compose(exported pair) against the call's own gst " + name, back, gst.astype(np.float64)) <= TOL


# ------------------------------------------------------------------ 3: styled call == reference-audio call
def _styled_against_reference(hp, w, tokens, tl, mels, ml, masks, noise, steps, persistent, **kw):
    B, Tv = tokens.shape
    _sole_context()
    m = _model(hp, w, B, mels.shape[1], Tv=Tv)
    style = m.Inference_GST_Step(mels, ml)
    runs = []
    for given in (False, True, False, True):        # capture and replay of both cached graphs, interleaved
        if given:
            out = m.Inference_Step(tokens, tl, None, prenet_masks=masks, attn_noise=noise, steps=steps, style_embeddings=style, **kw)
        else:
            out = m.Inference_Step(tokens, tl, None, mels, ml, prenet_masks=masks, attn_noise=noise, steps=steps, **kw)
        m.synchronize()
        runs.append(_np(*[t for t in out if t is not None]))
    if persistent:
        n, on = m.decode_counters()
        assert on == 1 and n >= 2, ("the persistent decode launch was not taken", n, on, m.last_message())
        assert m.handoff_error() == 0
    assert len(runs[0]) == (4 if kw.get("with_vocoder") else 3)
    assert _same("reference-audio call, replay", runs[0], runs[2])
    assert _same("styled call, replay", runs[1], runs[3])
    assert _same("styled call == reference-audio call (mel, stop, [spectrogram,] alignment)", runs[1], runs[0])
    return m


def _cfg2_call(B, seed, Tv=16, Tref=64, steps=4):
    from gst_tacotron_amd import synthetic
    rng = np.random.default_rng(seed)
    tokens, tl = synthetic.make_tokens(rng, B, Tv)
    lens = np.full(B, Tref, np.int32)
    lens[1] = 33
    mels, ml = synthetic.make_ref_mels(rng, B, Tref, lengths=lens)
    masks, noise = synthetic.make_randomness(rng, steps, B, Tv, [256, 256])
    return tokens, tl, mels, ml, masks, noise, steps


def test_styled_call_is_the_reference_audio_call_bitwise():
    """32 utterances x 16 tokens x 4 steps beside a 64-frame reference on the persistent decode launch."""
    hp, w = G.cfg2_weights()
    _styled_against_reference(hp, w, *_cfg2_call(32, 111), persistent=True)


def test_styled_call_is_the_reference_audio_call_bitwise_mixed_precision():
    hp, w = G.cfg2_weights()
    hp = copy.deepcopy(hp)
    hp["Use_Mixed_Precision"] = True
    _styled_against_reference(hp, w, *_cfg2_call(5, 112), persistent=False)


def test_styled_call_is_the_reference_audio_call_bitwise_masked_with_vocoder():
    hp, w, g = load_golden("tiny_sma_r2_gst")
    _styled_against_reference(hp, w, g["tokens"], g["token_lengths"], g["mels_for_gst"], g["mel_lengths_for_gst"], g["prenet_masks"],
                              g["attn_noise"], int(g["steps"]), persistent=False, masked=True, with_vocoder=True)


# ------------------------------------------------------------------ 4: interleaving on one model
def test_styled_and_reference_audio_calls_do_not_leak_into_each_other():
    """styled, reference-audio (its GST branch forked onto the side stream, 1024 frames: it outlasts the encoder convolutions), styled
    with another style: each is bitwise that call alone on a fresh model."""
    from gst_tacotron_amd import synthetic
    hp, w = G.cfg2_weights()
    B, Tv, Tref, steps = 8, 16, 1024, 4
    rng = np.random.default_rng(113)
    tokens, tl = synthetic.make_tokens(rng, B, Tv)
    lens = np.full(B, Tref, np.int32)
    lens[2], lens[5] = 577, 64
    mels, ml = synthetic.make_ref_mels(rng, B, Tref, lengths=lens)
    masks, noise = synthetic.make_randomness(rng, steps, B, Tv, [256, 256])
    A = S.dims(hp)[2]
    styles = [rng.standard_normal((B, A)).astype(np.float32) for _ in range(2)]
    kw = dict(prenet_masks=masks, attn_noise=noise, steps=steps)
    calls = [lambda m: m.Inference_Step(tokens, tl, None, style_embeddings=styles[0], **kw),
             lambda m: m.Inference_Step(tokens, tl, None, mels, ml, **kw),
             lambda m: m.Inference_Step(tokens, tl, None, style_embeddings=styles[1], **kw)]

    def run(m, call):
        mel, stop, _, align = call(m)       # (no synchronisation between the calls of the sequence: stream order alone)
        return mel, stop, align

    m = _model(hp, w, B, Tref + 1, Tv=Tv)
    seq = [run(m, c) for c in calls]
    m.synchronize()
    seq = [_np(*o) for o in seq]
    del m
    assert not np.array_equal(seq[0][0], seq[2][0]) and not np.array_equal(seq[0][0], seq[1][0])     # the style reaches the mel
    for i, c in enumerate(calls):
        fresh = _model(hp, w, B, Tref + 1, Tv=Tv)
        alone = run(fresh, c)
        fresh.synchronize()
        assert _same("call %d of the sequence == alone on a fresh model (mel, stop, alignment)" % i, seq[i], _np(*alone))
        del fresh


# ------------------------------------------------------------------ 5: token-conditioned whole call
def test_token_conditioned_call_is_the_composition_of_its_parts():
    hp, w = G.cfg2_weights()
    tokens, tl, _, _, masks, noise, steps = _cfg2_call(4, 114)
    B = tokens.shape[0]
    H, N, A = S.dims(hp)
    rng = np.random.default_rng(115)
    m = _model(hp, w, B, Tv=tokens.shape[1])
    style = m.Style_Compose(rng.uniform(-0.5, 1.0, (B, H, N)).astype(np.float32))
    mel, stop, _, align = m.Inference_Step(tokens, tl, None, prenet_masks=masks, attn_noise=noise, steps=steps, style_embeddings=style)
    whole = _np(mel, stop, align)
    pre, stop2, align2 = m.decode(m.encode(tokens), style, masks, noise, steps=steps)
    parts = _np(m.postnet(pre), stop2, align2)
    assert _same("Inference_Step(style) == decode(encode, style) + postnet (mel, stop, alignment)", whole, parts)
    # one style for the whole batch: [1, A] is that row tiled
    one = m.Style_Compose(rng.uniform(-0.5, 1.0, (1, H, N)).astype(np.float32))
    assert tuple(one.shape) == (1, A)
    a = m.Inference_Step(tokens, tl, None, prenet_masks=masks, attn_noise=noise, steps=steps, style_embeddings=one)
    b = m.Inference_Step(tokens, tl, None, prenet_masks=masks, attn_noise=noise, steps=steps, style_embeddings=one.repeat(B, 1))
    assert _same("[1, A] style == the row tiled", _np(a[0], a[1], a[3]), _np(b[0], b[1], b[3]))
    assert not np.array_equal(_np(a[0]), whole[0])


# ------------------------------------------------------------------ 6: Inference without any wav
def test_inference_from_token_weights_needs_no_wav(capsys):
    from gst_tacotron_amd import synthetic, weights
    hp = synthetic.tiny_hp()
    H, N, A = S.dims(hp)
    m = _model(hp, weights.synthetic_weights(hp, seed=5), 2, Tv=32)
    tw = np.zeros((H, N), np.float32)
    tw[:, 0] = 0.3                      # token 0 at weight 0.3 on every head, nothing else
    sentences = ["Hello there.", "Hi."]
    out = m.Inference(sentences, style_token_weights=tw)
    assert out is not None and "Inference fail" not in capsys.readouterr().out
    mel, stop, spec, align = out
    d = m.dims
    assert tuple(mel.shape) == (2, d.steps * d.r, d.mel) and tuple(stop.shape) == (2, d.steps) and spec is None
    assert tuple(align.shape) == (2, d.steps, len(sentences[0]) + 2)
    for t in (mel, stop, align):
        assert np.isfinite(_np(t)).all()
    # the same through the embedding
    again = m.Inference(sentences, style_embeddings=m.Style_Compose(tw[None]), seed=m.seed)
    assert np.array_equal(_np(again[0]), _np(mel))


# ------------------------------------------------------------------ 7: errors
def test_style_errors():
    from gst_tacotron_amd import capi, synthetic, weights
    hp = synthetic.tiny_hp()
    H, N, A = S.dims(hp)
    rng = np.random.default_rng(116)
    B, Tv = 2, 8
    m = _model(hp, weights.synthetic_weights(hp, seed=5), B, 9, Tv=Tv)
    tokens, tl = synthetic.make_tokens(rng, B, Tv)
    mels, ml = synthetic.make_ref_mels(rng, B, 8, mel=16)
    style = np.zeros((B, A), np.float32)
    with pytest.raises(ValueError, match="mutually exclusive"):
        m.Inference_Step(tokens, tl, None, mels, ml, style_embeddings=style, steps=2)
    for bad in (np.zeros((B, A + 1), np.float32), np.zeros((B + 1, A), np.float32), np.zeros((A,), np.float32),
                np.zeros((B, 1, A), np.float32)):
        with pytest.raises(ValueError, match="style_embeddings must be"):
            m.Inference_Step(tokens, tl, None, style_embeddings=bad, steps=2)
    for bad in (np.zeros((B, H, N + 1), np.float32), np.zeros((B, H + 1, N), np.float32), np.zeros((H, N), np.float32)):
        with pytest.raises(ValueError, match="token_weights must be"):
            m.Style_Compose(bad)
    with pytest.raises(ValueError, match="query must be"):
        m.Style_Compose(np.zeros((B, H, N), np.float32), np.zeros((B, A + 1), np.float32))
    with pytest.raises(capi.GstTacoError) as e:        # more rows than the capacity given at create
        m.Style_Compose(np.zeros((B + 1, H, N), np.float32))
    assert e.value.code == -5
    with pytest.raises(ValueError, match="mutually exclusive"):
        m.Inference(["Hi."], style_embeddings=style[:1], style_token_weights=np.zeros((H, N), np.float32))
    # the C-ABI itself refuses a NULL style
    import ctypes
    rc = m.ctx.lib.gsttaco_inference_step_styled(m.ctx.handle, None, None, None, None, None, ctypes.c_uint64(0), B, Tv, 2,
                                                 None, None, None, None, None, None)
    assert rc == -1
    # GST off
    hp0, w0, g = load_golden("tiny_sma_r1_nogst")
    m0 = _model(hp0, w0, g["tokens"].shape[0], Tv=g["tokens"].shape[1])
    with pytest.raises(ValueError, match="GST is not used"):
        m0.Inference_Step(g["tokens"], g["token_lengths"], None, style_embeddings=np.zeros((g["tokens"].shape[0], 16), np.float32))
    import torch
    buf = torch.zeros(64, device=m0.device)
    p = ctypes.c_void_p(buf.data_ptr())
    rc = m0.ctx.lib.gsttaco_inference_step_styled(m0.ctx.handle, p, None, p, None, None, ctypes.c_uint64(0), 1, 1, 1,
                                                  p, p, p, None, None, None)
    assert rc == -1 and "GST is not used" in m0.last_message()
    rc = m0.ctx.lib.gsttaco_style_compose(m0.ctx.handle, p, None, 1, p, None)
    assert rc == -1 and "GST is not used" in m0.last_message()
