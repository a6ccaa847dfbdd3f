"""GPU tests of the validation losses: gsttaco_losses (csrc/loss.hip) against the float64 restatement of tests/eval_cases.py,
gsttaco_feature_frontend's spectrogram against the float64 oracle at tests/audio_cases.py's Sound sections, Evaluate_Step against the
float64 forced oracle of tests/forced_cases.py, and Evaluate end to end on two synthetic wavs."""
import ctypes

import numpy as np
import pytest

import audio_cases as C
import eval_cases as E
import forced_cases as F
from gst_tacotron_amd import evaluate, hparams, synthetic
from oracle import oracle_np

pytestmark = pytest.mark.gpu

RTOL = E.RTOL


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _np(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _close(got, want, rtol=RTOL):
    """|got - want| <= rtol * |want| element by element (no absolute slack: an exact 0 must come back as 0)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64
    return bool((np.abs(got - want) <= rtol * np.abs(want)).all())


# ---------------------------------------------------------------------------------------------------- 1. the loss kernel
def _loss_model(sh):
    """A context with the shape's Mel_Dim / Spectrogram_Dim / Step_Reduction and room for its steps.  No Restore: no weights here."""
    from gst_tacotron_amd.model import GST_Tacotron
    S = E.n_steps(sh)
    if sh.mel == 80:
        hp = hparams.load_hp()
        hp["Step_Reduction"], hp["Max_Step"] = sh.r, S * sh.r
    else:
        hp = synthetic.tiny_hp(r=sh.r, max_step=S * sh.r)
    assert hp["Sound"]["Mel_Dim"] == sh.mel and (not sh.spec or hp["Sound"]["Spectrogram_Dim"] == sh.spec)
    return GST_Tacotron(hyper_parameters=hp, max_batch=sh.B, max_tokens=8, max_ref_frames=4, max_wav_seconds=0.0)


@pytest.mark.parametrize("name", list(E.SHAPES))
def test_loss_terms_equal_the_float64_restatement(name):
    """Random fp32 tensors at the smallest shapes at which the kernel can go wrong.  After the fp32 subtraction both sides are double
    and differ in summation order only (n * 2^-53, n <= 5.6e5: 6e-11), so rtol 1e-9 -- 60 x below one fp32 rounding -- holds and an
    fp32 accumulator fails it.  Two calls are bitwise equal; the prediction frames beyond T hold NaN and are never read."""
    sh, c, want = E.SHAPES[name], E.loss_case(name), E.loss_reference(name)
    m = _loss_model(sh)
    c = {k: None if v is None else np.array(v) for k, v in c.items()}          # (writable copies: torch warns about read-only arrays)
    args = (c["pre_mel"], c["mel"], c["stop"], c["teacher"], c["mel_lengths"], c["spec"], c["spec_target"], c["spec_lengths"])
    got, again = _np(m.Loss_Terms(*args), m.Loss_Terms(*args))
    rel = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
    print(name, "max relative error per field vs float64", rel.max(axis=0), "bound", RTOL)
    assert got.dtype == np.float64 and got.shape == (sh.B, 6) and np.isfinite(got).all()
    assert _close(got, want), (got, want)
    assert np.array_equal(got, again)
    if sh.spec:
        # without (either of) the spectrogram tensors fields 4 and 5 are exactly 0 and the rest is bitwise unchanged
        for spec, target in ((None, c["spec_target"]), (c["spec"], None), (None, None)):
            part = _np(m.Loss_Terms(*args[:5], spec, target, c["spec_lengths"]))[0]
            assert (part[:, 4:] == 0.0).all() and np.array_equal(part[:, :4], got[:, :4])
        # lengths NULL = T; lengths beyond T and below 0 are clipped (the stop labels use the length as given)
        full = _np(m.Loss_Terms(*args[:4], None, c["spec"], c["spec_target"], None))[0]
        assert _close(full, E.losses(c["pre_mel"], c["mel"], c["stop"], c["teacher"], sh.r, None, c["spec"], c["spec_target"], None))
        odd = np.array([sh.T + 5, -3, 2][:sh.B], np.int32)
        clipped = _np(m.Loss_Terms(*args[:4], odd, c["spec"], c["spec_target"], odd))[0]
        assert _close(clipped, E.losses(c["pre_mel"], c["mel"], c["stop"], c["teacher"], sh.r, odd, c["spec"], c["spec_target"], odd))
    # a non-finite input propagates -- to the fields of the row that reads it and nowhere else
    if sh.lengths is not None and sh.lengths[-1] > 0:
        b = sh.B - 1
        bad = np.array(c["mel"])
        bad[b, 0, 3] = np.inf
        g = _np(m.Loss_Terms(c["pre_mel"], bad, *args[2:]))[0]
        assert np.isinf(g[b, 1]) and np.isinf(g[b, 2]) and np.array_equal(g[b, [0, 3]], got[b, [0, 3]])
        assert np.array_equal(g[:b], got[:b])
        bad = np.array(c["stop"])
        bad[b, 0] = np.nan
        g = _np(m.Loss_Terms(c["pre_mel"], c["mel"], bad, *args[3:]))[0]
        assert np.isnan(g[b, 3]) and np.array_equal(np.delete(g, 3, 1), np.delete(got, 3, 1))


def test_losses_entry_point_contract():
    """Straight through the C ABI into a NaN-filled buffer one row longer than needed: every element of [B][6] is written, nothing
    behind it; the documented error codes."""
    import torch
    name = "trailing_frame"
    sh, c, want = E.SHAPES[name], E.loss_case(name), E.loss_reference(name)
    m = _loss_model(sh)
    S, Tq = E.n_steps(sh), sh.T + 1
    dev = lambda a, dt=torch.float32: None if a is None else torch.as_tensor(np.array(a), dtype=dt).to(m.device)
    t = {k: dev(v, torch.int32 if k.endswith("lengths") else torch.float32) for k, v in c.items()}
    out = torch.full((sh.B + 1, 6), float("nan"), dtype=torch.float64, device=m.device)
    lib, h = m.ctx.lib, m.ctx.handle

    def call(pre="pre_mel", mel="mel", stop="stop", teacher="teacher", B=sh.B, S=S, Tq=Tq, losses=out):
        g = lambda k: _ptr(t[k]) if k else None
        return lib.gsttaco_losses(h, g(pre), g(mel), g(stop), _ptr(t["spec"]), g(teacher), _ptr(t["spec_target"]), _ptr(t["mel_lengths"]),
                                  _ptr(t["spec_lengths"]), B, S, Tq, _ptr(losses), m._stream())
    assert call() == 0
    got = _np(out)[0]
    assert _close(got[:sh.B], want) and np.isnan(got[sh.B]).all()
    for k in ("pre", "mel", "stop", "teacher"):
        assert call(**{k: None}) == -1 and "null" in m.last_message()
    assert call(losses=None) == -1
    assert call(Tq=1) == -1 and call(S=S - 1) == -1 and call(B=0) == -1        # Tq < 2; S * r = 6 < Tq - 1 = 8
    assert call(B=sh.B + 1) == -5 and call(S=S + 1) == -5                      # beyond max_batch / Max_Step // r
    m.synchronize()


# ---------------------------------------------------------------------------------------------------- 2. the feature front end
def _audio_model(case, B=5):
    from gst_tacotron_amd.model import GST_Tacotron
    return GST_Tacotron(hyper_parameters=case.hp(), max_batch=B, max_tokens=8, max_ref_frames=4, max_wav_seconds=4.0)


def _features(m, case, wavs, top_db, want=("mels", "specs"), mel_only_entry=False, extra_frames=3):
    """gsttaco_feature_frontend (or gsttaco_mel_frontend) into NaN-filled buffers longer than needed -> (mels, specs, lengths)."""
    import torch
    B, ld = len(wavs), max(17, max(w.shape[0] for w in wavs))
    host = np.zeros((B, ld), np.float32)
    for i, w in enumerate(wavs):
        host[i, :w.shape[0]] = w
    wav = torch.from_numpy(host).to(m.device)
    lens = torch.tensor([w.shape[0] for w in wavs], dtype=torch.int32, device=m.device)
    cap = 2 + ld // case.hop + extra_frames
    mels = torch.full((B, cap, case.mel), float("nan"), dtype=torch.float32, device=m.device)
    specs = torch.full((B, cap, case.nb), float("nan"), dtype=torch.float32, device=m.device)
    out_len = torch.full((B,), -7, dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        if mel_only_entry:
            rc = m.ctx.lib.gsttaco_mel_frontend(m.ctx.handle, _ptr(wav), _ptr(lens), B, ld, ctypes.c_float(float(top_db)), _ptr(mels),
                                                _ptr(out_len), cap, m._stream())
        else:
            rc = m.ctx.lib.gsttaco_feature_frontend(m.ctx.handle, _ptr(wav), _ptr(lens), B, ld, ctypes.c_float(float(top_db)),
                                                    _ptr(mels) if "mels" in want else None, _ptr(specs) if "specs" in want else None,
                                                    _ptr(out_len), cap, m._stream())
    torch.cuda.synchronize()
    return rc, mels.cpu().numpy(), specs.cpu().numpy(), out_len.cpu().numpy()


@pytest.mark.parametrize("top_db", C.TOP_DBS)
@pytest.mark.parametrize("name", C.NAMES)
def test_feature_frontend_spectrogram_matches_the_oracle(name, top_db):
    """The five-row batch of tests/test_gpu_audio.py's front-end test: lengths are expected_frames, the mels are bitwise
    gsttaco_mel_frontend's, frame 0 and the padding are zero in both outputs up to cap_frames, and the spectrogram is within the
    project's bar for this kernel (mel_tol: its fp32 FFT and log10 against float64) of the float64 reference.  Measured on an MI355X,
    worst row per section: 4.4e-5, 9.7e-7 ([0, 1] scale, bar 2.5e-4), 1.5e-5 and, at nfft2048, 6.6e-4 (row 4, the burst just above
    n_fft / 2, at both top_db; rows 0 and 1 stay below 1.8e-4) against the bar of 2e-3; a float32 NumPy restatement with a
    mixed-radix FFT reaches 3.2e-4 there (tests/test_eval_cases.py)."""
    case = C.BY_NAME[name]
    wavs, refs = C.front_batch(name, top_db), E.spectrogram_reference(name, top_db)
    m = _audio_model(case)
    rc, mels, specs, lens = _features(m, case, wavs, top_db)
    assert rc == 0, m.last_message()
    assert not np.isnan(mels).any() and not np.isnan(specs).any(), "an element of an output buffer was never written"
    assert lens.tolist() == [C.expected_frames(case, w, top_db) for w in wavs] == [0 if r is None else r.shape[0] for r in refs]
    rc, only_mels, _, only_lens = _features(m, case, wavs, top_db, mel_only_entry=True)
    assert rc == 0 and np.array_equal(only_lens, lens)
    assert np.array_equal(mels, only_mels), "the mels differ from gsttaco_mel_frontend's"
    assert (mels[:, 0] == 0.0).all() and (specs[:, 0] == 0.0).all()
    worst = 0.0
    for i, ref in enumerate(refs):
        n = int(lens[i])
        assert (mels[i, 1 + n:] == 0.0).all() and (specs[i, 1 + n:] == 0.0).all(), ("padding of row", i)
        if ref is None:
            continue
        err = float(np.abs(specs[i, 1:1 + n].astype(np.float64) - ref).max())
        print(name, "top_db", top_db, "row", i, "frames", n, "spectrogram max abs err", err, "tolerance", case.mel_tol)
        worst = max(worst, err)
    assert worst <= case.mel_tol
    # either output alone: the same values; neither: an error
    rc, _, specs_alone, lens_alone = _features(m, case, wavs, top_db, want=("specs",))
    assert rc == 0 and np.array_equal(specs_alone, specs) and np.array_equal(lens_alone, lens)
    rc, mels_alone, _, _ = _features(m, case, wavs, top_db, want=("mels",))
    assert rc == 0 and np.array_equal(mels_alone, mels)
    assert _features(m, case, wavs, top_db, want=())[0] == -1
    # Feature_Generate on the rows Mel_Generate accepts: its mels are Mel_Generate's, bit for bit
    valid = [w for w, r in zip(wavs, refs) if r is not None]
    fm, fs, fl = _np(*m.Feature_Generate(valid, top_db))
    gm, gl = _np(*m.Mel_Generate(valid, top_db))
    keep = [i for i, r in enumerate(refs) if r is not None]
    assert np.array_equal(fm, gm) and np.array_equal(fl, gl) and fl.tolist() == lens[keep].tolist()
    assert fs.shape == (len(valid), 1 + int(fl.max()), case.nb)
    assert np.array_equal(fs[0, :1 + int(fl[0])], specs[keep[0], :1 + int(fl[0])])      # (row 0 is the longest wav: the same ld_wav)


# ---------------------------------------------------------------------------------------------------- 3. Evaluate_Step
def _variant(seed, mixed=False):
    """forced_cases.make_case(VARIANT) and the tokens / reference mels it drew (make_case keeps only what the oracle made of them)."""
    sh = F.VARIANT
    c = F.make_case(sh, seed=seed, mixed=mixed)
    rng = np.random.default_rng(seed)
    tokens, tl = synthetic.make_tokens(rng, sh.B, sh.Tv)
    mels, ml = synthetic.make_ref_mels(rng, sh.B, 12)
    w64 = oracle_np.cast_weights(c.w, np.float64)
    assert np.array_equal(oracle_np.encoder(c.hp, w64, tokens, np.float64), c.enc)
    return c, w64, tokens, tl, mels, ml


def _postnet(c, w64, pre, mixed):
    prev, oracle_np.MIXED = oracle_np.MIXED, mixed
    try:
        return oracle_np.postnet(c.hp, w64, pre, np.float64)
    finally:
        oracle_np.MIXED = prev


@pytest.mark.parametrize("mixed", [False, True], ids=["fp32", "mixed"])
def test_evaluate_step_against_the_forced_oracle(mixed):
    """forced_cases.VARIANT (5 x 48 tokens, r = 2, Tq = 12: T = 11, S = 6, S * r = 12 > T) with injected randomness and ragged mel
    lengths.  The sums are eval_cases.losses of the call's own outputs (rtol 1e-9).  Against the float64 forced oracle: L1 and the bce
    are 1-Lipschitz in each prediction, so fields 0 and 1 are within L * TOL and field 3 within S * TOL of the oracle's, with TOL the
    project's bar on those predictions (forced_cases.TOL; MIXED_TOL under Use_Mixed_Precision); |a^2 - b^2| <= |a - b| (2 |b| + |a - b|)
    puts field 2 within L * TOL * (2 max|d| + TOL), d the oracle's difference."""
    from gst_tacotron_amd.model import GST_Tacotron
    tol = F.MIXED_TOL if mixed else F.TOL
    c, w64, tokens, tl, mels, ml = _variant(131, mixed)
    sh, r, S = F.VARIANT, F.VARIANT.r, c.S
    T = sh.Tq - 1
    lengths = np.array([11, 7, 1, 10, 4], np.int32)
    spec_lengths = np.array([11, 6, 2, 9, 4], np.int32)
    spec_dim = c.hp["Sound"]["Spectrogram_Dim"]
    spec_target = np.clip(np.random.default_rng(5).normal(0.0, 1.5, (sh.B, sh.Tq, spec_dim)), -4.0, 4.0).astype(np.float32)
    m = GST_Tacotron(hyper_parameters=c.hp, max_batch=sh.B, max_tokens=sh.Tv, max_ref_frames=13)
    m.Restore(weights=c.w)
    sums, out = m.Evaluate_Step(tokens, tl, c.teacher, lengths, spec_target, spec_lengths, mels_for_gst=mels, mel_lengths_for_gst=ml,
                                prenet_masks=c.masks, attn_noise=c.noise)
    sums, mel, stop, spec, align, pre = _np(sums, *out)
    assert sums.shape == (sh.B, 6) and sums.dtype == np.float64 and spec.shape == (sh.B, S * r, spec_dim) and pre.shape == mel.shape
    own = E.losses(pre, mel, stop, c.teacher, r, lengths, spec, spec_target, spec_lengths)
    assert _close(sums, own), (sums, own)
    assert (sums > 0).all()
    rp, rs, ra = F.reference(c, mixed=mixed)
    rmel = _postnet(c, w64, rp, mixed)
    print("max abs err of the predictions vs the oracle: pre", np.abs(pre - rp).max(), "mel", np.abs(mel - rmel).max(), "stop",
          np.abs(stop - rs).max(), "bar", tol)
    want = E.losses(rp, rmel, rs, c.teacher, r, lengths)
    L = np.clip(lengths, 0, T).astype(np.float64)
    dmax = np.array([np.abs(c.teacher[b, 1:1 + int(L[b])] - rmel[b, :int(L[b])]).max() for b in range(sh.B)])
    # (the restatement rounds the oracle's float64 predictions to fp32 before its one fp32 subtraction: 2^-24 * 8 per element more)
    slack = 2.0 ** -21
    bounds = {0: L * (tol + slack), 1: L * (tol + slack), 2: L * (tol + slack) * (2 * dmax + tol + slack), 3: S * (tol + slack)}
    for f, bound in bounds.items():
        err = np.abs(sums[:, f] - want[:, f])
        print(E.FIELDS[f], "abs err vs the oracle's loss", err, "bound", bound)
        assert (err <= bound).all(), (E.FIELDS[f], err, bound)
    if not mixed:
        # no style given: the teacher itself with the mel lengths is the style input (Model.py:206), go frame and padding included
        kw = dict(prenet_masks=c.masks, attn_noise=c.noise)
        a, _ = m.Evaluate_Step(tokens, tl, c.teacher, lengths, **kw)
        b, _ = m.Evaluate_Step(tokens, tl, c.teacher, lengths, mels_for_gst=c.teacher, mel_lengths_for_gst=lengths, **kw)
        a, b = _np(a, b)
        assert np.array_equal(a, b) and (a[:, 4:] == 0).all() and not np.array_equal(a[:, :4], sums[:, :4])
        with pytest.raises(ValueError, match="sets"):
            m.Evaluate_Step(tokens, tl, c.teacher, lengths, steps=3)


# ---------------------------------------------------------------------------------------------------- 4. Evaluate
def test_evaluate_end_to_end_on_two_synthetic_wavs():
    """synthetic.tiny_hp() (GST, r = 2, a vocoder) on two short two-tone signals: the spectrogram term is there, ``loss`` is
    ``combine`` of ``per_utterance``, the same seeds give the same numbers, and a row equals that utterance evaluated alone.

    Alone means: the same style embedding (the reference encoder looks past an utterance's length into the batch's padding) and, for
    the SHORTER row, field 0 only -- the pre-net mel of a teacher-forced decoder is causal, but the post-net (five convolutions of
    width 5) and the CBHG vocoder (a bidirectional RNN) of the inference graph run over all S * r frames, so a row's mel and
    spectrogram below its length depend on how far the batch is padded beyond it.  The LONGEST row has the batch's own padding when
    run alone: all six fields.  The bound is that of tests/test_gpu_report.py's alone-vs-batch tests (TOL per prediction), carried
    through the 1-Lipschitz terms as in the test above."""
    from gst_tacotron_amd import weights
    from gst_tacotron_amd.model import GST_Tacotron
    hp = synthetic.tiny_hp(max_step=64)
    case = C.Case("tiny", 33, 64, 16, 16, 4)
    assert all(hp["Sound"][k] == v for k, v in case.sound.items())
    wavs = [C.signal(case, 640, 21), C.signal(case, 420, 22)]
    sentences = ["Hi there.", "Ok"]
    m = GST_Tacotron(hyper_parameters=hp, max_batch=2, max_tokens=16, max_ref_frames=64, max_wav_seconds=1.0)
    m.Restore(weights=weights.synthetic_weights(hp, seed=4))
    seeds = [11, 2 ** 40 + 5]
    res = m.Evaluate(sentences, wavs, seeds=seeds)
    assert set(res) == {"pre_mel", "mel", "stop", "spectrogram", "loss", "per_utterance", "mel_lengths", "steps"}
    per, lens, S = res["per_utterance"], res["mel_lengths"], res["steps"]
    fm, fs, fl = _np(*m.Feature_Generate(wavs, 15))
    assert lens.tolist() == fl.tolist() and lens[0] > lens[1] > 2
    T = -(-(int(lens.max()) + 1) // 2) * 2
    assert S == T // 2 and per.shape == (2, 6) and per.dtype == np.float64 and np.isfinite(per).all()
    assert res["spectrogram"] > 0 and (per[:, 4] > 0).all()
    want = evaluate.combine(per, T, S, False)
    assert all(res[k] == want[k] for k in want) and res["loss"] == res["pre_mel"] + res["mel"] + res["stop"] + res["spectrogram"]
    l2 = m.Evaluate(sentences, wavs, seeds=seeds, use_l2=True)
    assert np.array_equal(l2["per_utterance"], per) and l2["mel"] > res["mel"] and l2["pre_mel"] == res["pre_mel"]
    again = m.Evaluate(sentences, wavs, seeds=seeds)
    assert np.array_equal(again["per_utterance"], per) and again["loss"] == res["loss"]
    other = m.Evaluate(sentences, wavs, seeds=[12, 13])
    assert not np.array_equal(other["per_utterance"][:, :4], per[:, :4])            # (dropout is live: another draw, another loss)
    # mels (and spectrograms) given as arrays: the same numbers as from the wavs
    targets = [fm[i, 1:1 + int(fl[i])] for i in range(2)]
    spec_targets = [fs[i, 1:1 + int(fl[i])] for i in range(2)]
    from_arrays = m.Evaluate(sentences, targets, spec_targets, seeds=seeds)
    assert np.array_equal(from_arrays["per_utterance"], per)
    no_spec = m.Evaluate(sentences, targets, seeds=seeds)
    assert no_spec["spectrogram"] == 0.0 and np.array_equal(no_spec["per_utterance"][:, :4], per[:, :4])
    # a row against the utterance alone
    pat = m.feeder.Get_Evaluation_Pattern(sentences, targets, spec_targets)
    style = m.Inference_GST_Step(pat["teacher_mels"], pat["mel_lengths"])
    styled = m.Evaluate(sentences, targets, spec_targets, seeds=seeds, style_embeddings=style)["per_utterance"]
    assert np.array_equal(styled, per)                  # (the style Evaluate computes itself is that of the padded teacher)
    sums, out = m.Evaluate_Step(**pat, seeds=seeds, masked=True, style_embeddings=style)
    sums, mel, stop, spec = _np(sums, *out[:3])
    assert np.array_equal(sums, per)                    # (Evaluate is Evaluate_Step on the feeder's pattern)
    tol = F.TOL
    for b, fields in ((0, range(6)), (1, (0,))):
        one = m.Evaluate(sentences[b:b + 1], targets[b:b + 1], spec_targets[b:b + 1], seeds=seeds[b:b + 1],
                         style_embeddings=style[b:b + 1])
        n = int(lens[b])
        assert one["steps"] == (S if b == 0 else -(-(int(lens[1]) + 1) // 2)) and (b == 0 or one["steps"] < S)
        d_mel = float(np.abs(pat["teacher_mels"][b, 1:1 + n] - mel[b, :n]).max())
        d_spec = float(np.abs(pat["spectrograms"][b, 1:1 + n] - spec[b, :n]).max())
        bounds = {0: n * tol, 1: n * tol, 2: n * tol * (2 * d_mel + tol), 3: S * tol, 4: n * tol, 5: n * tol * (2 * d_spec + tol)}
        for f in fields:
            err = abs(one["per_utterance"][0, f] - per[b, f])
            print("row", b, E.FIELDS[f], "batch", per[b, f], "alone", one["per_utterance"][0, f], "abs diff", err, "bound", bounds[f])
            assert err <= bounds[f], (b, f, err, bounds[f])
    with pytest.raises(ValueError, match="one target"):
        m.Evaluate(sentences, wavs[:1])
    with pytest.raises(ValueError, match="spectrogram_List"):
        m.Evaluate(sentences, wavs, spec_targets)
