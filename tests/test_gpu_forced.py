"""GPU tests of teacher-forced decoding (gsttaco_decode_forced / gsttaco_inference_step_forced / gsttaco_forced_durations) against the
float64 forced decoder of tests/forced_cases.py, at the reference's decoder sizes and a handful of steps."""
import gc
import os

import numpy as np
import pytest

import forced_cases as F
from oracle import oracle_np

pytestmark = pytest.mark.gpu

TOL, MIXED_TOL = F.TOL, F.MIXED_TOL
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model(hp, w, B, Tv, Tref1=2, **kw):
    from gst_tacotron_amd.model import GST_Tacotron
    m = GST_Tacotron(hyper_parameters=hp, max_batch=max(B, 1), max_tokens=Tv, max_ref_frames=max(Tref1, 2), **kw)
    m.Restore(weights=w)
    return m


def _np(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _decode(m, c, **kw):
    """decode(..., teacher_mels=) from the oracle's encoder output and style embedding, injected randomness unless told otherwise."""
    kw.setdefault("prenet_masks", c.masks)
    kw.setdefault("attn_noise", c.noise)
    return _np(*m.decode(c.enc.astype(np.float32), c.gst.astype(np.float32), teacher_mels=c.teacher,
                         token_lengths=c.token_lengths, **kw))


def _assert_close(got, ref, tol, what):
    errs = {k: float(np.abs(g - r).max()) for k, g, r in zip(("pre_mel", "stop", "align"), got, ref)}
    print(what, "max abs err vs the float64 forced oracle", errs)
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.isfinite(g).all()
    assert max(errs.values()) <= tol, (what, errs)


@pytest.mark.parametrize("name", list(F.SHAPES))
def test_forced_decode_shapes_match_the_oracle(name):
    shape = F.SHAPES[name]
    c = F.make_case(shape, seed=300 + len(name))
    m = _model(c.hp, c.w, shape.B, shape.Tv)
    got = _decode(m, c)
    assert got[0].shape == (shape.B, c.S * shape.r, 80) and got[1].shape == (shape.B, c.S) and got[2].shape == (shape.B, c.S, shape.Tv)
    _assert_close(got, F.reference(c), TOL, name)
    assert m.decode_counters()[0] == 0 and m.handoff_error() == 0


def test_forced_decode_masked_ragged_token_lengths():
    c = F.make_case(F.MASKED, seed=41, token_lengths=np.array([33, 9, 20, 32], np.int32))
    m = _model(c.hp, c.w, F.MASKED.B, F.MASKED.Tv)
    got = _decode(m, c)
    _assert_close(got, F.reference(c), TOL, "masked")
    for b, n in enumerate(c.token_lengths):
        assert not got[2][b][:, n:].any()


@pytest.mark.parametrize("front", ["0", "1", None], ids=["four-kernel", "general-fused", "default"])
def test_forced_decode_front_end_variants(monkeypatch, front):
    if front is None:
        monkeypatch.delenv("GSTTACO_FUSED_FRONT", raising=False)
    else:
        monkeypatch.setenv("GSTTACO_FUSED_FRONT", front)
    c = F.make_case(F.VARIANT, seed=51)
    m = _model(c.hp, c.w, F.VARIANT.B, F.VARIANT.Tv)
    assert m.decode_plan(F.VARIANT.Tv)[0] is (front != "0")
    _assert_close(_decode(m, c), F.reference(c), TOL, "GSTTACO_FUSED_FRONT=" + str(front))
    assert m.decode_counters()[0] == 0


def test_forced_decode_hashed_dropout_is_the_free_runs_randomness():
    """A seed and no masks: the keep decisions and the noise of step t are what a free run draws at step t under that seed -- read
    back (gsttaco_debug_randomness) after each and compared, then fed to the oracle."""
    c = F.make_case(F.VARIANT, seed=61)
    B, Tv = F.VARIANT.B, F.VARIANT.Tv
    m = _model(c.hp, c.w, B, Tv)
    got = _decode(m, c, prenet_masks=None, attn_noise=None, seed=777)
    masks, noise = m.debug_randomness(c.S, B, Tv)
    assert set(np.unique(masks)) <= {0.0, 1.0} and 0.4 < masks.mean() < 0.6
    _assert_close(got, F.reference(c, masks=masks, noise=noise), TOL, "hashed")
    m.decode(c.enc.astype(np.float32), c.gst.astype(np.float32), seed=777, steps=c.S)
    masks2, noise2 = m.debug_randomness(c.S, B, Tv)
    assert np.array_equal(masks, masks2) and np.array_equal(noise, noise2)


def test_forced_decode_on_a_zero_padded_decoder():
    sizes = (128, 512, 64)
    c = F.make_case(F.VARIANT, seed=71, sizes=sizes)
    m = _model(c.hp, c.w, F.VARIANT.B, F.VARIANT.Tv)
    _assert_close(_decode(m, c), F.reference(c), TOL, "padded decoder")


def test_forced_decode_mixed_precision():
    """bf16 GEMM operands as tests/test_gpu_parity.py::_mixed_case sets them up; the Z0 product keeps fp32 operands, which is what
    oracle_np.prenet computes."""
    c = F.make_case(F.Shape(5, 40, 2, 21, "SMA"), seed=81, mixed=True)
    m = _model(c.hp, c.w, 5, 40)
    _assert_close(_decode(m, c), F.reference(c, mixed=True), MIXED_TOL, "mixed")


def test_forced_on_a_free_runs_frames_is_that_free_run():
    """Fixed point.  Not bitwise: the free run's prenet-0 pre-activations are the composed [h2|ctx].(Wp.W0) form."""
    shape = F.Shape(4, 33, 2, 17, "SMA")
    c = F.make_case(shape, seed=91)
    m = _model(c.hp, c.w, shape.B, shape.Tv)
    enc, gst = c.enc.astype(np.float32), c.gst.astype(np.float32)
    free = _np(*m.decode(enc, gst, c.masks, c.noise, steps=8))
    w64 = oracle_np.cast_weights(c.w, np.float64)
    ref = oracle_np.decoder(c.hp, w64, c.memory, np.float64, c.masks.astype(np.float64), c.noise.astype(np.float64), steps=8)
    _assert_close(free, ref, TOL, "free run")
    teacher = F.behind_go_frame(free[0])
    forced = _np(*m.decode(enc, gst, c.masks, c.noise, teacher_mels=teacher))
    _assert_close(forced, F.reference(c, teacher=teacher), TOL, "forced on the free run's frames")
    gap = [float(np.abs(a - b).max()) for a, b in zip(forced, free)]
    print("forced vs free", gap)
    assert max(gap) <= 2 * TOL, gap


def test_forced_graph_replay_is_bitwise_the_eager_launches(monkeypatch):
    c = F.make_case(F.VARIANT, seed=101)
    outs = []
    for graph in ("1", "0"):
        monkeypatch.setenv("GSTTACO_GRAPH", graph)
        m = _model(c.hp, c.w, F.VARIANT.B, F.VARIANT.Tv)
        first = _decode(m, c)
        again = _decode(m, c)                   # (with graphs: the replay of what the first call captured)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        assert (m.graph_cache_size() > 0) is (graph == "1")
        outs.append(again)
        del m
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_forced_calls_do_not_disturb_the_persistent_free_run():
    """free, forced, free, forced, free on the process's one context at 32 x 128: the persistent decode launch is what the free runs take,
    the forced calls in between take the launch path and change nothing for them.  decode_counters()[0] counts ENQUEUES of the
    persistent launch (eager, or into a graph being captured; a replay adds none), so the context captures a key at its second
    use (the policy callers with varying lengths are told to use): the free run after the forced call is enqueued afresh, and which
    form that enqueue took is what the counter shows."""
    from gst_tacotron_amd import synthetic
    gc.collect()
    B, Tv, Tref, steps = 32, 128, 20, 6
    hp, w = F.full_weights("SMA", 2)
    rng = np.random.default_rng(7)
    tokens, tl = synthetic.make_tokens(rng, B, Tv)
    mels, ml = synthetic.make_ref_mels(rng, B, Tref)
    teacher = F.make_teacher(rng, B, 1 + 2 * steps)
    m = _model(hp, w, B, Tv, Tref + 1)
    m.set_graph_policy(max_cached=16, capture_after=2)
    run = lambda **kw: _np(*[t for t in m.Inference_Step(tokens, tl, None, mels, ml, seed=5, **kw) if t is not None])
    a = run(steps=steps)                            # eager
    n0, on = m.decode_counters()
    assert on == 1 and n0 >= 1, m.last_message()
    f1 = run(teacher_mels=teacher)                  # eager
    assert m.decode_counters()[0] == n0 and np.isfinite(f1[0]).all() and f1[0].shape == a[0].shape
    assert not np.array_equal(f1[0], a[0])
    b = run(steps=steps)                            # second use: captured, i.e. enqueued again -- behind a forced call
    n1, on = m.decode_counters()
    assert n1 > n0 and on == 1 and m.handoff_error() == 0
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    cache = m.graph_cache_size()
    f2 = run(teacher_mels=teacher)                  # second use: captured
    assert m.decode_counters()[0] == n1
    assert m.graph_cache_size() == cache + 1        # (the forced middle segment only: the encoder segment's graph is the free run's)
    assert all(np.array_equal(x, y) for x, y in zip(f1, f2))
    c = run(steps=steps)                            # replay of the free run's graphs
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    assert m.decode_counters() == (n1, 1) and m.graph_cache_size() == cache + 1 and m.handoff_error() == 0
    m.synchronize()


def test_forced_inference_step_from_mels_and_from_a_style_embedding():
    """The whole call with the vocoder on synthetic.tiny_hp(): against the oracle's pipeline around the forced decoder, and the call
    with Inference_GST_Step's embedding is bitwise the call with the reference mels."""
    from gst_tacotron_amd import synthetic, weights
    hp = synthetic.tiny_hp("SMA", r=2, gst=True, max_step=24)
    w = weights.synthetic_weights(hp, seed=4)
    rng = np.random.default_rng(8)
    B, Tv, Tref, Tq = 3, 12, 30, 16
    S = F.n_steps(Tq, 2)
    tokens, tl = synthetic.make_tokens(rng, B, Tv)
    mels, ml = synthetic.make_ref_mels(rng, B, Tref, mel=16, lengths=np.array([30, 11, 17]))
    masks, noise = synthetic.make_randomness(rng, S, B, Tv, [32, 32])
    teacher = F.make_teacher(rng, B, Tq, mel=16)
    m = _model(hp, w, B, Tv, Tref + 1)
    kw = dict(prenet_masks=masks, attn_noise=noise, with_vocoder=True, return_pre_mel=True, teacher_mels=teacher)
    from_mels = _np(*m.Inference_Step(tokens, tl, None, mels, ml, **kw))
    style = m.Inference_GST_Step(mels, ml)
    from_style = _np(*m.Inference_Step(tokens, tl, style_embeddings=style, **kw))
    for a, b in zip(from_mels, from_style):
        assert np.array_equal(a, b)
    mel, stop, spec, align, pre = from_mels
    assert mel.shape == (B, S * 2, 16) and spec.shape == (B, S * 2, 33) and stop.shape == (B, S) and align.shape == (B, S, Tv)
    w64 = oracle_np.cast_weights(w, np.float64)
    enc = oracle_np.encoder(hp, w64, tokens, np.float64)
    gst = oracle_np.style_token_layer(hp, w64, mels, ml, np.float64)
    rp, rs, ra = F.forced_decoder(hp, w64, oracle_np.gst_concat(enc, gst), teacher, np.float64, masks, noise)
    rmel = oracle_np.postnet(hp, w64, rp, np.float64)
    rspec = oracle_np.vocoder_taco1(hp, w64, rmel, np.float64)
    _assert_close((pre, stop, align), (rp, rs, ra), TOL, "Inference_Step(teacher_mels=)")
    assert np.abs(mel - rmel).max() <= TOL and np.abs(spec - rspec).max() <= TOL
    with pytest.raises(ValueError, match="steps"):
        m.Inference_Step(tokens, tl, None, mels, ml, teacher_mels=teacher, steps=4)
    with pytest.raises(ValueError, match="teacher_mels"):
        m.Inference_Step(tokens, tl, None, mels, ml, teacher_mels=teacher[:, :, :8])
    with pytest.raises(ValueError, match="teacher_mels"):
        m.decode(enc.astype(np.float32), gst.astype(np.float32), teacher_mels=teacher[:2])


def test_forced_durations_equal_the_numpy_count():
    import torch
    c = F.make_case(F.MASKED, seed=111)
    B, Tv, r = F.MASKED.B, F.MASKED.Tv, F.MASKED.r
    m = _model(c.hp, c.w, B, 150)
    align = m.decode(c.enc.astype(np.float32), c.gst.astype(np.float32), c.masks, c.noise, teacher_mels=c.teacher)[2]
    a = _np(align)[0]
    S = c.S
    tl = np.array([33, 9, 20, 1], np.int32)
    for tok, mel_len in ((None, None), (tl, None), (None, np.array([S * r, 7, 1, 0], np.int32)),      # lengths that are no multiple of r, 0
                         (tl, np.array([S * r + 5, 3, S * r - 1, 8], np.int32))):                     # a length beyond S * r
        d = _np(m.Forced_Durations(align, tok, mel_len))[0]
        want = F.durations(a, r, tok, mel_len)
        assert d.dtype == np.int32 and np.array_equal(d, want), (tok, mel_len)
        L = np.full(B, S * r) if mel_len is None else np.minimum(mel_len, S * r)
        assert d.sum(1).tolist() == L.tolist()
    # ties: the lowest index wins, also across the lanes of the wave that scans a row and beyond its first 64 columns
    tie = np.zeros((2, 3, 150), np.float32)
    tie[0, 0, [70, 5, 133]] = 1.0
    tie[0, 1, [149, 64]] = 2.0
    tie[1, 2, 100] = -1.0                       # all other columns 0 > -1: column 0
    d = _np(m.Forced_Durations(torch.from_numpy(tie)))[0]
    assert np.array_equal(d, F.durations(tie, r)) and d[0, 5] == r and d[0, 64] == r and d[0, 0] == r and d[1, 0] == 3 * r


def test_forced_error_paths():
    from gst_tacotron_amd import capi
    shape = F.Shape(2, 16, 2, 6, "SMA")
    c = F.make_case(shape, seed=121)
    hp = dict(c.hp); hp["Max_Step"] = 8          # 4 steps
    m = _model(hp, c.w, 2, 16, 4)
    enc, gst = c.enc.astype(np.float32), c.gst.astype(np.float32)
    ok = m.decode(enc, gst, c.masks, c.noise, teacher_mels=c.teacher)
    assert ok[0].shape == (2, 6, 80)
    import ctypes
    import torch
    dev = lambda a, dt=torch.float32: torch.as_tensor(a, dtype=dt).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    e_, g_, t_ = dev(enc), dev(gst), dev(c.teacher)
    pre, stop, align = torch.empty(2, 8, 80).cuda(), torch.empty(2, 4).cuda(), torch.empty(2, 4, 16).cuda()
    lib, h = m.ctx.lib, m.ctx.handle

    def dec(teacher, Tq, B=2, Tv=16):
        return lib.gsttaco_decode_forced(h, p(e_), p(g_), None, None, None, ctypes.c_uint64(1), B, Tv, p(teacher), Tq,
                                         p(pre), p(stop), p(align), None)
    assert dec(None, 6) == -1 and "teacher" in m.last_message()
    assert dec(t_, 1) == -1
    assert dec(t_, 10) == -5                     # S = 5 > Max_Step // r = 4
    assert dec(t_, 6, B=3) == -5 and dec(t_, 6, Tv=17) == -5
    assert dec(t_, 6) == 0
    tok = dev(np.zeros((2, 16)), torch.int32)
    mels = dev(np.zeros((2, 4, 80)))
    ml = dev(np.array([3, 3]), torch.int32)
    mel_out = torch.empty(2, 8, 80).cuda()

    def step(mels_, style_, teacher=t_, Tq=6):
        return lib.gsttaco_inference_step_forced(h, p(tok), None, p(mels_), p(ml), p(style_), None, None, ctypes.c_uint64(1), 2, 16, 4,
                                                 p(teacher), Tq, p(mel_out), p(stop), p(align), None, None, None)
    assert step(mels, g_) == -1 and step(None, None) == -1              # both / neither style source
    assert step(mels, None, teacher=None) == -1 and step(None, g_, Tq=1) == -1 and step(None, g_, Tq=10) == -5
    assert step(mels, None) == 0 and step(None, g_) == 0
    torch.cuda.synchronize()
    with pytest.raises(capi.GstTacoError) as e:
        m.decode(enc, gst, teacher_mels=np.zeros((2, 10, 80), np.float32))
    assert e.value.code == -5
    dur = torch.empty(2, 16, dtype=torch.int32).cuda()
    assert lib.gsttaco_forced_durations(h, None, None, None, 2, 4, 16, p(dur), None) == -1
    assert lib.gsttaco_forced_durations(h, p(align), None, None, 2, 4, 17, p(dur), None) == -5
    assert lib.gsttaco_forced_durations(h, p(align), None, None, 2, 4, 16, p(dur), None) == 0
    m.synchronize()


def test_inference_gta_end_to_end_on_two_fixture_signals():
    """Two of the committed signals (tests/golden/audio_synth_full.npz, the shipped Sound section) as GTA targets: wavs through the GPU
    mel front end, the style from the same audio, trimmed mels and durations back -- against the oracle's pipeline on the mels and the
    randomness the device used."""
    import json
    from gst_tacotron_amd.model import GST_Tacotron
    g = np.load(os.path.join(GOLD, "audio_synth_full.npz"))
    sigs = [g["sig3"], g["sig4"]]
    lens = [g["mel3_15"].shape[0], g["mel4_15"].shape[0]]
    hp, w = F.full_weights("SMA", 2)
    assert json.loads(str(g["sound_json"])) == {k: hp["Sound"][k] for k in json.loads(str(g["sound_json"]))}     # the shipped Sound section
    sentences = ["Hi there.", "Ok"]
    m = GST_Tacotron(hyper_parameters=hp, max_batch=2, max_tokens=16, max_ref_frames=64, max_wav_seconds=1.0)
    m.Restore(weights=w)
    gta, stop, align, dur = m.Inference_GTA(sentences, sigs, seed=9)
    assert [tuple(x.shape) for x in gta] == [(n, 80) for n in lens]
    pat = m.feeder.Get_Inference_Pattern(sentences, style_given=True)
    tokens, tl = pat["tokens"], pat["token_lengths"]
    B, Tv = tokens.shape
    dmel, dlen = m.Mel_Generate(sigs, 15)
    dmel, dlen = _np(dmel, dlen)
    assert dlen.tolist() == lens
    teacher = m.feeder.Get_Teacher_Pattern(sentences, [dmel[i, 1:1 + n] for i, n in enumerate(lens)])["teacher_mels"]
    S = F.n_steps(teacher.shape[1], 2)
    masks, noise = m.debug_randomness(S, B, Tv)
    stop, align, dur = _np(stop, align, dur)
    assert stop.shape == (B, S) and align.shape == (B, S, Tv) and dur.sum(1).tolist() == lens
    assert np.array_equal(dur, F.durations(align, 2, tl, np.array(lens)))
    w64 = oracle_np.cast_weights(w, np.float64)
    ref_mels = np.zeros((B, max(lens) + 1, 80), np.float32)
    for i, n in enumerate(lens):
        ref_mels[i, 1:n + 1] = dmel[i, 1:n + 1]
    enc = oracle_np.encoder(hp, w64, tokens, np.float64)
    gst = oracle_np.style_token_layer(hp, w64, ref_mels, np.array(lens), np.float64)
    rp, rs, ra = F.forced_decoder(hp, w64, oracle_np.gst_concat(enc, gst), teacher, np.float64, masks, noise)
    rmel = oracle_np.postnet(hp, w64, rp, np.float64)
    assert np.abs(align - ra).max() <= TOL and np.abs(stop - rs).max() <= TOL
    for i, n in enumerate(lens):
        assert np.abs(_np(gta[i])[0] - rmel[i, :n]).max() <= TOL
