"""CPU: the restatements of tests/eval_cases.py add up to the reference's Train_Step, the feeder's evaluation layout is the reference's
training batch, the new C symbols are declared and exported, and the spectrogram cases are well conditioned in float32."""
import os

import numpy as np
import pytest

import audio_cases as C
import eval_cases as E
from gst_tacotron_amd import capi, evaluate, hparams
from gst_tacotron_amd.feeder import Feeder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(rng, B, T, r, mel, spec, lengths, spec_lengths):
    """A padded training batch with T a multiple of r (what Feeder.py:134-143 builds) and random logits: float32."""
    assert T % r == 0
    def target(ch, lens):
        a = np.zeros((B, T + 1, ch), np.float32)
        for b, n in enumerate(lens):
            a[b, 1:1 + n] = np.clip(rng.normal(0.0, 1.5, (n, ch)), -4.0, 4.0)
        return a
    logit = lambda ch: rng.normal(0.0, 1.5, (B, T, ch)).astype(np.float32)
    return dict(mels=target(mel, lengths), spectrograms=target(spec, spec_lengths), pre=logit(mel), mel=logit(mel), spec=logit(spec),
                stop=rng.normal(0.0, 3.0, (B, T // r)).astype(np.float32), mel_lengths=np.array(lengths, np.int32),
                spec_lengths=np.array(spec_lengths, np.int32))


@pytest.mark.parametrize("use_l2", [False, True])
@pytest.mark.parametrize("r,T,lengths,spec_lengths", [
    (1, 7, (7, 1, 4), (7, 1, 4)),
    (3, 9, (9, 7, 1), (8, 9, 3)),           # spectrogram lengths that differ from the mel lengths
    (2, 12, (10, 3, 12, 1), (11, 2, 12, 5)),
])
def test_combined_sums_are_the_train_step_reduction(use_l2, r, T, lengths, spec_lengths):
    rng = np.random.default_rng(17 * r + T)
    B = len(lengths)
    g = _batch(rng, B, T, r, 16, 33, lengths, spec_lengths)
    sums = E.losses(g["pre"], g["mel"], g["stop"], g["mels"], r, g["mel_lengths"], g["spec"], g["spectrograms"], g["spec_lengths"])
    got = evaluate.combine(sums, T, T // r, use_l2)
    want = E.train_step_loss(g["mels"], g["mel_lengths"], g["pre"], g["mel"], g["stop"], r, g["spectrograms"], g["spec_lengths"],
                             g["spec"], use_l2)
    assert set(got) == {"pre_mel", "mel", "stop", "spectrogram", "loss"}
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (k, got[k], want[k])
    assert got["spectrogram"] > 0 and got["loss"] == got["pre_mel"] + got["mel"] + got["stop"] + got["spectrogram"]
    # without spectrograms the term is 0 and the rest is unchanged
    sums0 = E.losses(g["pre"], g["mel"], g["stop"], g["mels"], r, g["mel_lengths"])
    got0 = evaluate.combine(sums0, T, T // r, use_l2)
    want0 = E.train_step_loss(g["mels"], g["mel_lengths"], g["pre"], g["mel"], g["stop"], r, use_l2=use_l2)
    assert got0["spectrogram"] == 0.0 and abs(got0["loss"] - want0["loss"]) <= 1e-12 * max(1.0, abs(want0["loss"]))
    assert (got["mel"] > evaluate.combine(sums, T, T // r, False)["mel"]) is use_l2
    assert got["pre_mel"] == evaluate.combine(sums, T, T // r, not use_l2)["pre_mel"]       # the L2 field never enters pre_mel


def test_padding_dilutes_the_frame_terms_and_per_utterance_means_do_not():
    """The reference's quirk, kept: the same utterance in a batch padded to twice the length reports half the frame terms."""
    rng = np.random.default_rng(3)
    g = _batch(rng, 1, 6, 2, 16, 33, (6,), (6,))
    sums = E.losses(g["pre"], g["mel"], g["stop"], g["mels"], 2, g["mel_lengths"])
    a, b = evaluate.combine(sums, 6, 3), evaluate.combine(sums, 12, 3)
    assert abs(a["mel"] - 2 * b["mel"]) <= 1e-15 and abs(a["pre_mel"] - 2 * b["pre_mel"]) <= 1e-15 and a["stop"] == b["stop"]
    means = evaluate.per_utterance_means(sums, [6])
    assert abs(means[0, 1] - a["mel"]) <= 1e-15 and means[0, 3] == sums[0, 3]
    assert (evaluate.per_utterance_means(np.zeros((2, 6)), [0, 3]) == 0.0).all()
    assert evaluate.per_utterance_means(sums, [6], steps=3)[0, 3] == sums[0, 3] / 3
    with pytest.raises(ValueError):
        evaluate.combine(np.zeros((2, 5)), 4, 2)
    assert evaluate.use_l2_of(hparams.load_hp()) is False and evaluate.use_l2_of({"Train": {"Use_L2_Loss": True}}) is True
    assert evaluate.LOSS_FIELDS == E.FIELDS


def test_stable_bce_equals_the_naive_formula_where_that_is_finite():
    x = np.concatenate([np.linspace(-30, 30, 121), [-100.0, 100.0, -745.0, 745.0, 0.0]])
    for z in (0.0, 1.0):
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            naive = E.bce_naive(x, z)
        stable = E.bce(x, z)
        assert np.isfinite(stable).all() and (stable >= 0).all()
        ok = np.isfinite(naive)
        assert ok[:121].all()                       # |x| <= 30: the naive form is finite ...
        # ... but not exact: s is rounded to 2^-53, so log(s) / log(1 - s) are off by up to 2^-53 / min(s, 1 - s) = 2^-53 (1 + e^|x|)
        bound = 4 * 2.0 ** -53 * (1.0 + np.exp(np.abs(x[:121]))) + 1e-14 * stable[:121]
        assert (np.abs(stable[:121] - naive[:121]) <= bound).all()
        assert not ok.all()                         # ... and beyond it overflows on one side, where the stable form is exact
    assert E.bce(100.0, 0.0) == 100.0 and E.bce(-100.0, 1.0) == 100.0 and 0 < E.bce(100.0, 1.0) < 1e-40
    c = E.loss_case(E.BIG_LOGITS)
    assert np.abs(c["stop"]).max() == 100.0 and np.isfinite(E.loss_reference(E.BIG_LOGITS)).all()


def test_loss_cases_cover_their_rows():
    assert list(E.SHAPES) == ["odd_channels", "label_edges", "trailing_frame", "empty_row", "long"]
    for name, sh in E.SHAPES.items():
        c, ref = E.loss_case(name), E.loss_reference(name)
        S = E.n_steps(sh)
        assert c["stop"].shape == (sh.B, S) and c["teacher"].shape == (sh.B, sh.T + 1, sh.mel) and ref.shape == (sh.B, 6)
        assert np.isfinite(ref).all(), name         # (the NaN prediction frames beyond T are never read)
        assert (c["spec"] is None) == (sh.spec == 0) and (ref[:, 4:] == 0).all() == (sh.spec == 0)
    sh = E.SHAPES["trailing_frame"]
    assert E.n_steps(sh) * sh.r == sh.T + 1 and np.isnan(E.loss_case("trailing_frame")["mel"][:, sh.T:]).all()
    ref = E.loss_reference("empty_row")
    assert (ref[0, [0, 1, 2]] == 0).all() and ref[0, 3] > 0 and (ref[1] > 0)[:4].all()
    assert [-(-n // 3) for n in E.SHAPES["label_edges"].lengths] == [3, 3, 1]
    assert E.SHAPES["long"].T > 1024


def test_evaluation_pattern_is_the_reference_training_layout():
    hp = hparams.load_hp()
    rng = np.random.default_rng(5)
    mel_dim, spec_dim = hp["Sound"]["Mel_Dim"], hp["Sound"]["Spectrogram_Dim"]
    for r, mel_T, spec_T in ((2, (5, 9), (5, 9)), (3, (4, 7), (11, 6)), (1, (6, 2), (3, 6)), (2, (8, 3), (2, 3))):
        hp["Step_Reduction"] = r
        mels = [rng.normal(size=(n, mel_dim)).astype(np.float32) for n in mel_T]
        specs = [rng.normal(size=(n, spec_dim)).astype(np.float32) for n in spec_T]
        f = Feeder(hp)
        pat = f.Get_Evaluation_Pattern(["Hi there.", "Ok"], mels, specs)
        want_m, want_s = E.evaluation_layout(mels, specs, r)
        assert np.array_equal(pat["teacher_mels"], want_m) and np.array_equal(pat["spectrograms"], want_s)
        assert pat["teacher_mels"].shape[1] == pat["spectrograms"].shape[1] and (pat["teacher_mels"].shape[1] - 1) % r == 0
        assert pat["mel_lengths"].tolist() == list(mel_T) and pat["spectrogram_lengths"].tolist() == list(spec_T)
        assert pat["mel_lengths"].dtype == np.int32 and pat["spectrogram_lengths"].dtype == np.int32
        teach = f.Get_Teacher_Pattern(["Hi there.", "Ok"], mels)
        assert np.array_equal(pat["tokens"], teach["tokens"]) and np.array_equal(pat["token_lengths"], teach["token_lengths"])
        plain = f.Get_Evaluation_Pattern(["Hi there.", "Ok"], mels)
        assert set(plain) == set(teach) and np.array_equal(plain["teacher_mels"], teach["teacher_mels"])
    with pytest.raises(ValueError):
        f.Get_Evaluation_Pattern(["Hi there.", "Ok"], mels, specs[:1])
    with pytest.raises(ValueError):
        f.Get_Evaluation_Pattern(["Hi there.", "Ok"], mels, [s[:, :5] for s in specs])


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    for sym in ("gsttaco_losses", "gsttaco_feature_frontend"):
        assert ("int " + sym + "(") in header and sym in capi.EXPORTED_SYMBOLS
    assert "double* losses" in header and capi.ABI_VERSION == 14
    from gst_tacotron_amd import build
    assert "loss.hip" in build.SOURCES


@pytest.mark.parametrize("top_db", C.TOP_DBS)
@pytest.mark.parametrize("name", C.NAMES)
def test_spectrogram_cases_are_well_conditioned_in_float32(name, top_db):
    """The float32 restatement of the kernel's pipeline stays under a quarter of the tolerance the GPU test uses: the case table, not
    the kernel, would fail first."""
    case = C.BY_NAME[name]
    refs = E.spectrogram_reference(name, top_db)
    worst = 0.0
    for wav, ref, mel_ref in zip(C.front_batch(name, top_db), refs, C.front_reference(name, top_db)):
        assert (ref is None) == (mel_ref is None)
        if ref is None:
            continue
        assert ref.shape[0] == mel_ref.shape[0]
        lo, hi = (0.0, 1.0) if case.max_abs is None else (-case.max_abs, case.max_abs)
        assert ref.min() >= lo and ref.max() <= hi
        got = E.spectrogram_float32(case, wav, top_db)
        worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
    print(name, "top_db", top_db, "float32 restatement vs float64: max abs err", worst, "bar", case.mel_tol / 4)
    assert worst <= case.mel_tol / 4
