"""GPU tests of per-utterance seeds and the synthesis report (csrc/report.hip: gsttaco_fill_randomness, gsttaco_utterance_report) and of
what is built on them (``seeds=``, ``Utterance_Report``, ``Inference_Checked``), against tests/report_cases.py."""
import copy
import ctypes

import numpy as np
import pytest

import forced_cases as F
import report_cases as R
from gst_tacotron_amd import checked, export, synthetic, weights

pytestmark = pytest.mark.gpu

TOL = F.TOL
NOISE_TOL = 4.45e-6                 # tests/test_gpu_rng.py's bound on the device's Box-Muller against float64
SEEDS = [0x9E3779B97F4A7C15, (0xDEADBEEF << 32) | 17, (1 << 63) + 5]          # high words set
LENS = np.array([12, 5, 9], np.int32)


def _np(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _full_model(rate=0.5, B=3, Tv=70):
    from gst_tacotron_amd.model import GST_Tacotron
    hp, w = F.full_weights("SMA", 2)
    hp = copy.deepcopy(hp)
    hp["Tacotron2"]["Decoder"]["Prenet"]["Dropout_Rate"] = rate
    m = GST_Tacotron(hyper_parameters=hp, max_batch=B, max_tokens=Tv, max_ref_frames=2)
    m.Restore(weights=w)
    return m


@pytest.fixture(scope="module")
def full():
    """cfg2's sizes (prenet 256 / 256, SMA, r = 2, dropout 0.5), 3 utterances x 70 tokens; the tokens and styles the tests share."""
    m = _full_model()
    rng = np.random.default_rng(77)
    tokens, _ = synthetic.make_tokens(rng, 3, 12, lengths=LENS)
    style = rng.normal(0.0, 0.5, (3, m.dims.gst_att)).astype(np.float32)
    yield m, tokens, style
    m.ctx.close()


def _weightless(max_step, B, Tv, prenet=None):
    """A created context without weights: all the two entry points need."""
    from gst_tacotron_amd.model import GST_Tacotron
    hp = synthetic.tiny_hp("SMA", r=2, gst=True, max_step=max_step)
    if prenet:
        hp["Tacotron2"]["Decoder"]["Prenet"]["Size"] = list(prenet)
    return GST_Tacotron(hyper_parameters=hp, max_batch=B, max_tokens=Tv)


# ---------------------------------------------------------------------------------------------------- the fill kernel
@pytest.mark.parametrize("rate", [0.5, 0.25], ids=["hash", "philox"])
def test_fill_is_the_batch_of_one_randomness_of_each_seed(rate, full):
    import torch
    steps, Tv = 5, 70
    m = full[0] if rate == 0.5 else _full_model(rate)
    masks, noise = m.Fill_Randomness(SEEDS, steps, Tv)
    assert tuple(masks.shape) == (steps, 2, 3, 256) and tuple(noise.shape) == (steps, 3, Tv)
    masks, noise = _np(masks, noise)
    rm, rn = R.randomness(SEEDS, steps, Tv, 256, rate)
    print(rate, "masks: keep fraction", float(masks.mean()), "; elements differing from the restatement", int((masks != rm).sum()))
    assert np.array_equal(masks, rm)
    err = float(np.abs(noise.astype(np.float64) - rn).max())
    print(rate, "noise: max abs error against float64 Box-Muller", err, "; max |noise|", float(np.abs(noise).max()), "; bound", NOISE_TOL)
    assert np.isfinite(noise).all() and err <= NOISE_TOL
    # row b IS what a batch of one draws under seed = seeds[b]
    rng = np.random.default_rng(5)
    tokens, _ = synthetic.make_tokens(rng, 1, Tv)
    style = rng.normal(0.0, 0.5, (1, m.dims.gst_att)).astype(np.float32)
    for b, seed in enumerate(SEEDS):
        m.Inference_Step(tokens, style_embeddings=style, seed=seed, steps=steps)
        torch.cuda.synchronize()
        one_m, one_n = m.debug_randomness(steps, 1, Tv)
        assert np.array_equal(one_m[:, :, 0], masks[:, :, b]) and np.array_equal(one_n[:, 0], noise[:, b]), b
    # ... whatever the width, the row order and the batch size
    m12, n12 = _np(*m.Fill_Randomness(SEEDS, steps, 12))
    assert np.array_equal(m12, masks) and np.array_equal(n12, noise[:, :, :12])
    mp, npm = _np(*m.Fill_Randomness([SEEDS[2], SEEDS[0]], steps, Tv))
    assert np.array_equal(mp, masks[:, :, [2, 0]]) and np.array_equal(npm, noise[:, [2, 0]])
    # seeds are taken mod 2^64; the high word counts
    mw, nw = _np(*m.Fill_Randomness([s + (1 << 64) for s in SEEDS], steps, Tv))
    assert np.array_equal(mw, masks) and np.array_equal(nw, noise)
    ml, _ = _np(*m.Fill_Randomness([s & 0xFFFFFFFF for s in SEEDS], steps, Tv))
    assert not np.array_equal(ml, masks)


# ---------------------------------------------------------------------------------------------------- invariance
def _alone(m, tokens, style, b, seed, **kw):
    n = int(LENS[b])
    mel, stop, align = _np(*[t for t in m.Inference_Step(tokens[b:b + 1, :n], style_embeddings=style[b:b + 1], seed=seed, **kw)
                             if t is not None])
    return mel[0], stop[0], align[0]


def _assert_rows_are_the_utterances_alone(m, tokens, style, got, seeds, what, **kw):
    mel, stop, align = got
    for b in range(3):
        n = int(LENS[b])
        one = _alone(m, tokens, style, b, seeds[b], **kw)
        errs = [float(np.abs(one[0] - mel[b]).max()), float(np.abs(one[1] - stop[b]).max()), float(np.abs(one[2] - align[b][:, :n]).max())]
        print(what, "row", b, "vs the utterance alone under its seed: max abs diff mel / stop / align", errs)
        assert max(errs) <= TOL, (what, b, errs)
        assert not align[b][:, n:].any()


def test_seeded_rows_equal_the_utterance_alone_whatever_the_batch(full):
    """The throughput-mode twin of test_config3_batch128_variable_length_with_padding_masks: generated randomness, the hashed front on
    the single-seed side."""
    m, tokens, style = full
    steps = 12
    run = lambda **kw: _np(*[t for t in m.Inference_Step(tokens, LENS, style_embeddings=style, steps=steps, masked=True, **kw)
                             if t is not None])
    mel, stop, align = run(seeds=SEEDS)
    assert mel.shape == (3, steps * 2, 80) and np.isfinite(mel).all()
    _assert_rows_are_the_utterances_alone(m, tokens, style, (mel, stop, align), SEEDS, "seeds", steps=steps)
    order = [2, 0, 1]
    pm, ps, pa = _np(*[t for t in m.Inference_Step(tokens[order], LENS[order], style_embeddings=style[order], steps=steps, masked=True,
                                                   seeds=[SEEDS[i] for i in order]) if t is not None])
    perm = [float(np.abs(pm - mel[order]).max()), float(np.abs(ps - stop[order]).max()), float(np.abs(pa - align[order]).max())]
    print("permuted batch vs permuted outputs", perm)
    assert max(perm) <= TOL, perm
    # one seed for the whole batch: row 0 draws what it draws alone, rows 1 and 2 do not -- the property is the seeds', not the masking's
    sm, ss, sa = run(seed=SEEDS[0])
    diff = [float(np.abs(sm[b] - mel[b]).max()) for b in range(3)]
    print("one seed vs seeds, max abs mel diff per row", diff)
    assert diff[0] <= TOL and diff[1] > 100 * TOL and diff[2] > 100 * TOL, diff
    with pytest.raises(ValueError, match="seeds"):
        m.Inference_Step(tokens, LENS, style_embeddings=style, steps=steps, masked=True, seeds=SEEDS, seed=1)
    with pytest.raises(ValueError, match="seeds"):
        m.Inference_Step(tokens, LENS, style_embeddings=style, steps=steps, masked=True, seeds=SEEDS[:2])


def test_seeded_forced_rows_equal_the_forced_utterance_alone(full):
    m, tokens, style = full
    teacher = F.make_teacher(np.random.default_rng(9), 3, 12)           # S = 6 (Tq - 1 = 11 is not a multiple of r)
    got = _np(*[t for t in m.Inference_Step(tokens, LENS, style_embeddings=style, masked=True, seeds=SEEDS, teacher_mels=teacher)
                if t is not None])
    assert got[1].shape == (3, 6)
    mel, stop, align = got
    for b in range(3):
        n = int(LENS[b])
        one = _alone(m, tokens, style, b, SEEDS[b], teacher_mels=teacher[b:b + 1])
        errs = [float(np.abs(one[0] - mel[b]).max()), float(np.abs(one[1] - stop[b]).max()), float(np.abs(one[2] - align[b][:, :n]).max())]
        print("forced row", b, "vs alone", errs)
        assert max(errs) <= TOL, (b, errs)


# ---------------------------------------------------------------------------------------------------- the report kernel
def _report(m, stop, align, tl=None, mel=None):
    """gsttaco_utterance_report straight through the C-ABI into buffers holding a sentinel."""
    import torch
    dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    B, S, Tv = align.shape
    st, al, tl_, ml = dev(stop, torch.float32), dev(align, torch.float32), dev(tl, torch.int32), dev(mel, torch.float32)
    rep = torch.full((B + 1, 8), -77, dtype=torch.int32).cuda()
    foc = torch.full((B + 1,), -77.0).cuda()
    rc = m.ctx.lib.gsttaco_utterance_report(m.ctx.handle, p(st), p(al), p(tl_), p(ml), B, S, Tv, p(rep), p(foc), None)
    assert rc == 0, m.last_message()
    rep, foc = _np(rep, foc)
    assert (rep[B] == -77).all() and foc[B] == -77.0            # nothing behind the last row
    return rep[:B], foc[:B]


def _assert_report(m, stop, align, r, tl=None, mel=None, what=""):
    rep, foc = _report(m, stop, align, tl, mel)
    want, wfoc = R.report(stop, align, r, tl, mel)
    print(what, "report\n", rep, "\nfocus", foc, "float64", wfoc)
    assert rep.dtype == np.int32 and np.array_equal(rep, want), (what, rep, want)
    ulp = np.spacing(np.abs(wfoc).astype(np.float32)).astype(np.float64)
    assert (np.abs(foc.astype(np.float64) - wfoc) <= ulp).all(), (what, foc, wfoc)
    return rep, foc


def _stops(rng, B, S, first):
    """Positive logits with stop[b, first[b]] < 0 (first[b] == S: never) and arbitrary signs behind it."""
    stop = rng.uniform(0.1, 3.0, (B, S)).astype(np.float32)
    for b, f in enumerate(first):
        if f < S:
            stop[b, f] = -0.5
            stop[b, f + 1:] = rng.normal(0.0, 1.0, S - f - 1)
    return stop


TL = np.array([150, 1, 64, 65, 7], np.int32)


def test_report_matches_the_restatement_on_synthetic_tensors():
    rng = np.random.default_rng(31)
    B, S, Tv, r, mel_dim = 5, 13, 150, 2, 16
    m = _weightless(2 * S, B, Tv)
    align = rng.random((B, S, Tv)).astype(np.float32)
    # row 3: a monotonic walk that stalls over steps 2..5, the stop at step 7 and a back step behind it that must not count
    align[3] = R.one_hot_path([0, 20, 40, 40, 40, 40, 63, 64, 30, 64, 64, 10, 64], Tv)[0]
    # row 4: ties -- across lanes and beyond column 64 (the lowest index wins), a whole row tied
    align[4] = 0.0
    align[4, 0, [70, 5, 133]] = 1.0
    align[4, 1, [149, 64]] = 2.0
    align[4, 2, 100] = -1.0
    align[4, 3:, 6] = 0.5
    first = [0, S, 6, 7, S]
    stop = _stops(rng, B, S, first)
    mel = rng.normal(0.0, 1.0, (B, S * r, mel_dim)).astype(np.float32)
    mel[2, 6 * r - 1, 3] = np.inf               # row 2's frame frames - 1: counts
    mel[2, 6 * r, 0] = np.inf                   # its frame `frames`: does not
    mel[0, 2, 0] = np.nan                       # row 0 (s* = 0): frames = r = 2, frame 2 lies behind them
    for tl in (None, TL):
        rep, _ = _assert_report(m, stop, align, r, tl, None, "no mel, token_lengths %s" % (tl is not None))
        assert rep[:, 0].tolist() == first and rep[:, 1].tolist() == [2, 26, 12, 14, 26] and not rep[:, 7].any()
        if tl is None:
            assert rep[3].tolist() == [7, 14, 149 - 63, 23, 0, 4, 4, 0]
            assert rep[4, 2:7].tolist() == [149 - 64, 59, 1, S - 3, 4]      # 5, 64, 0, 6, 6, ...
        else:
            assert rep[1, 2:7].tolist() == [0, 0, 0, S, 1]              # n = 1
            assert rep[4, 2:7].tolist() == [0, 6, 1, S - 3, 3]          # n = 7: 5, 0, 0, 6, 6, ...
        rep, _ = _assert_report(m, stop, align, r, tl, mel, "mel, token_lengths %s" % (tl is not None))
        assert rep[:, 7].tolist() == [0, 0, 1, 0, 0]
    # non-finite stop logits and alignments: counted in front of the stop and below the token length only; fields 0 and 1 still hold
    stop2, align2 = stop.copy(), align.copy()
    stop2[2, 1] = np.nan                        # not below 0: the stop stays at step 6
    stop2[2, 9] = np.inf                        # behind the stop
    align2[3, 2, 64] = np.inf                   # column 64 = n - 1 of row 3
    align2[3, 2, 65] = np.nan                   # column n: counted only without token_lengths
    align2[3, 9, 0] = np.nan                    # behind the stop
    for tl, cnt in ((None, 2), (TL, 1)):
        rep, _ = _report(m, stop2, align2, tl)
        want, _ = R.report(stop2, align2, r, tl)
        assert np.array_equal(rep[:, [0, 1, 7]], want[:, [0, 1, 7]]) and rep[:, 7].tolist() == [0, 0, 1, cnt, 0]
        assert np.array_equal(rep[[0, 1, 4]], want[[0, 1, 4]])
    # the method: the same numbers as device tensors
    drep, dfoc = m.Utterance_Report(stop, align, TL, mel)
    assert drep.is_cuda and tuple(drep.shape) == (B, 8) and tuple(dfoc.shape) == (B,)
    drep, dfoc = _np(drep, dfoc)
    rep, foc = _report(m, stop, align, TL, mel)
    assert np.array_equal(drep, rep) and np.array_equal(dfoc, foc)


def test_report_of_a_single_step():
    rng = np.random.default_rng(32)
    m = _weightless(2, 2, 150)
    align = rng.random((2, 1, 150)).astype(np.float32)
    for stop in (np.array([[-1.0], [1.0]], np.float32), np.array([[0.0], [np.nan]], np.float32)):
        rep, _ = _report(m, stop, align, np.array([150, 70], np.int32))
        want, _ = R.report(stop, align, 2, np.array([150, 70]))
        assert np.array_equal(rep, want)
        assert rep[:, 1].tolist() == [2, 2] and rep[:, 3:7].tolist() == [[0, 0, 1, 1]] * 2
    _assert_report(m, np.array([[-1.0], [1.0]], np.float32), align, 2, None, None, "S = 1")


def test_report_over_a_thousand_steps():
    """More steps than the kernel keeps in the LDS at once (512): runs, jumps and back steps across the boundary between two chunks."""
    rng = np.random.default_rng(33)
    S, Tv = 1000, 8
    m = _weightless(2 * S, 1, Tv)
    align = rng.random((1, S, Tv)).astype(np.float32)
    align[0, 505:520] = R.one_hot_path([3] * 15, Tv)[0]                 # a stall over steps 505..519
    never = np.ones((1, S), np.float32)
    rep, _ = _assert_report(m, never, align, 2, None, None, "S = 1000")
    assert rep[0, 0] == S and rep[0, 1] == 2 * S and rep[0, 5] >= 15
    rep, _ = _assert_report(m, _stops(rng, 1, S, [700]), align, 2, np.array([5], np.int32), None, "S = 1000, stop at 700")
    assert rep[0, 0] == 700
    # the stall ends exactly with the first chunk / begins exactly with the second; a back step and a jump right on the boundary
    for path in ([1] * 500 + [6] * 12 + [2] * 488, [1] * 500 + [2] * 12 + [6] * 488, [4] * 512 + [0] * 488, [5] * S):
        a = R.one_hot_path(path, Tv)
        rep, _ = _assert_report(m, never, a, 2, None, None, "paths")
    assert rep[0, 2:7].tolist() == [2, 0, 0, S, 1]
    rep, _ = _assert_report(m, _stops(rng, 1, S, [512]), R.one_hot_path([4] * 512 + [0] * 488, Tv), 2, None, None, "stop at 512")
    assert rep[0].tolist() == [512, 1024, 3, 0, 0, 512, 1, 0]


def test_fill_and_report_error_paths():
    import torch
    m = _weightless(8, 2, 16)                   # 4 steps
    lib, h = m.ctx.lib, m.ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    seeds = torch.tensor([1, 2], dtype=torch.int64).cuda()
    masks, noise = torch.empty(4, 2, 2, max(m.dims.prenet)).cuda(), torch.empty(4, 2, 16).cuda()
    fill = lambda s, mk, nz, B=2, Tv=16, steps=4: lib.gsttaco_fill_randomness(h, p(s), B, Tv, steps, p(mk), p(nz), None)
    assert fill(None, masks, noise) == -1 and "null" in m.last_message()
    assert fill(seeds, None, None) == -1
    assert fill(seeds, masks, noise, B=0) == -1
    assert fill(seeds, masks, noise, B=3) == -5 and fill(seeds, masks, noise, Tv=17) == -5 and fill(seeds, masks, noise, steps=5) == -5
    assert fill(seeds, masks, noise) == 0 and fill(seeds, masks, None) == 0 and fill(seeds, None, noise) == 0
    stop, align = torch.ones(2, 4).cuda(), torch.rand(2, 4, 16).cuda()
    rep, foc = torch.empty(2, 8, dtype=torch.int32).cuda(), torch.empty(2).cuda()
    report = lambda st, al, rp, B=2, S=4, Tv=16, f=foc: lib.gsttaco_utterance_report(h, p(st), p(al), None, None, B, S, Tv, p(rp), p(f), None)
    assert report(None, align, rep) == -1 and report(stop, None, rep) == -1 and report(stop, align, None) == -1
    assert report(stop, align, rep, S=0) == -1
    assert report(stop, align, rep, B=3) == -5 and report(stop, align, rep, S=5) == -5 and report(stop, align, rep, Tv=17) == -5
    assert report(stop, align, rep) == 0 and report(stop, align, rep, f=None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="stops"):
        m.Utterance_Report(stop[:, :3], align)
    # unequal prenet layers: the stacked mask layout does not exist -- the noise alone still does
    u = _weightless(8, 2, 16, prenet=(32, 16))
    assert u.ctx.lib.gsttaco_fill_randomness(u.ctx.handle, p(seeds), 2, 16, 4, p(masks), p(noise), None) == -1
    assert "equal prenet" in u.last_message()
    assert u.ctx.lib.gsttaco_fill_randomness(u.ctx.handle, p(seeds), 2, 16, 4, None, p(noise), None) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- on real decodes
def test_report_of_a_real_decode_and_its_frames_in_griffin_lim():
    import torch
    from gst_tacotron_amd.model import GST_Tacotron
    hp = synthetic.tiny_hp("SMA", r=2, gst=True, max_step=24)
    w = weights.synthetic_weights(hp, seed=4)
    rng = np.random.default_rng(8)
    B, Tv = 3, 12
    tokens, tl = synthetic.make_tokens(rng, B, Tv, lengths=np.array([12, 7, 10]))
    mels, ml = synthetic.make_ref_mels(rng, B, 30, mel=16)
    m = GST_Tacotron(hyper_parameters=hp, max_batch=B, max_tokens=Tv, max_ref_frames=31, max_wav_seconds=1.0)
    m.Restore(weights=w)
    mel, stop, spec, align = m.Inference_Step(tokens, tl, None, mels, ml, seed=11, masked=True, with_vocoder=True)
    rep, foc = m.Utterance_Report(stop, align, tl, mel)
    h_mel, h_stop, h_align, h_rep, h_foc = _np(mel, stop, align, rep, foc)
    want, wfoc = R.report(h_stop, h_align, 2, tl, h_mel)
    print("decode report\n", h_rep, "\nfocus", h_foc)
    assert np.array_equal(h_rep, want) and not h_rep[:, 7].any()
    assert (np.abs(h_foc.astype(np.float64) - wfoc) <= np.spacing(np.abs(wfoc).astype(np.float32))).all()
    # Export_Inference's host path: .cpu() the stop logits, slice per utterance, frames = max(1, s*) * r
    frames = np.array([max(1, export.stop_slice_index(s)) * 2 for s in h_stop], np.int32)
    assert h_rep[:, 1].tolist() == frames.tolist()
    wav_h, len_h = _np(*m.Inv_Spectrogram(spec, frames=frames, iters=3, seed=5))
    wav_d, len_d = _np(*m.Inv_Spectrogram(spec, frames=rep[:, 1], iters=3, seed=5))
    assert np.array_equal(len_h, len_d) and np.array_equal(wav_h, wav_d)


def test_inference_checked_redoes_only_the_rejected_rows(tmp_path):
    import torch
    from gst_tacotron_amd.model import GST_Tacotron
    hp, w = F.full_weights("SMA", 2)
    hp = copy.deepcopy(hp)
    hp["Inference_Path"] = str(tmp_path)
    sentences = ["Hi there.", "Ok", "Hello."]
    steps, seeds = 6, [SEEDS[0], (1 << 64) - 2, 7]
    m = GST_Tacotron(hyper_parameters=hp, max_batch=3, max_tokens=16, max_ref_frames=2)
    m.Restore(weights=w)
    m.set_graph_policy(max_cached=16, capture_after=2)
    style = np.random.default_rng(3).normal(0.0, 0.5, (3, m.dims.gst_att)).astype(np.float32)
    step, batches = m.Inference_Step, []

    def counted(*a, **kw):
        batches.append((kw["tokens"].shape, list(kw["seeds"])))
        assert kw["masked"] is True
        return step(*a, **kw)
    m.Inference_Step = counted
    reject, judged = {(0, 0), (2, 0), (2, 1)}, []

    def accept(row, focus, i, k):
        judged.append((i, k))
        assert len(row) == 8 and row[1] == max(1, row[0]) * 2 and 0.0 < focus <= 1.0
        return (i, k) not in reject
    mels, report, focus, attempts, stops, aligns = m.Inference_Checked(sentences, style_embeddings=style, seeds=seeds, max_attempts=3,
                                                                       accept=accept, steps=steps)
    m.Inference_Step = step
    pat = m.feeder.Get_Inference_Pattern(sentences, style_given=True)
    tokens, tl = pat["tokens"], pat["token_lengths"]
    Tv = tokens.shape[1]
    assert attempts.tolist() == [1, 0, 2]
    assert [b[0] for b in batches] == [(3, Tv), (2, int(tl[[0, 2]].max())), (1, int(tl[2]))]
    assert batches[1][1] == [checked.attempt_seed(seeds[0], 1), checked.attempt_seed(seeds[2], 1)]
    assert batches[2][1] == [checked.attempt_seed(seeds[2], 2)]
    assert judged == [(0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (2, 2)]
    report, focus, stops, aligns = _np(report, focus, stops, aligns)
    assert stops.shape == (3, steps) and aligns.shape == (3, steps, Tv)
    assert [int(x.shape[0]) for x in mels] == report[:, 1].tolist()
    for i in range(3):
        n = int(tl[i])
        mel, stop, _, align = step(tokens[i:i + 1, :n], style_embeddings=style[i:i + 1], steps=steps,
                                   seed=checked.attempt_seed(seeds[i], int(attempts[i])))
        mel, stop, align = _np(mel, stop, align)
        errs = [float(np.abs(_np(mels[i])[0] - mel[0, :report[i, 1]]).max()), float(np.abs(stops[i] - stop[0]).max()),
                float(np.abs(aligns[i][:, :n] - align[0]).max())]
        print("checked row", i, "attempt", int(attempts[i]), "vs the sentence alone under its derived seed", errs)
        assert max(errs) <= TOL, (i, errs)
        assert not aligns[i][:, n:].any()
    want, wfoc = R.report(stops, aligns, 2, tl)                  # the returned report is the returned tensors'
    assert np.array_equal(report[:, :7], want[:, :7]) and not report[:, 7].any()
    assert (np.abs(focus.astype(np.float64) - wfoc) <= np.spacing(np.abs(wfoc).astype(np.float32))).all()
    with pytest.raises(ValueError, match="itself"):
        m.Inference_Checked(sentences, style_embeddings=style, seed=3)
