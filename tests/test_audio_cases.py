"""CPU: the inputs of tests/test_gpu_audio.py are well conditioned and can see what they are meant to see (no GPU involved: these are
properties of the cases in tests/audio_cases.py and of the float64 oracle, not of the kernels)."""
import numpy as np
import pytest

import audio_cases as C
from oracle import audio_np as A


def test_tolerances_are_the_existing_ones():
    import test_audio
    assert C.MEL_TOL == test_audio.MEL_TOL == 2e-3 and C.GL_TOL == 2e-3


def test_cases_leave_the_tested_sections_where_they_claim():
    by = C.BY_NAME
    assert [(c.n_fft, c.win, c.hop, c.mel, c.max_abs, c.sr) for c in C.CASES] == [
        (64, 48, 16, 16, 4, 16000), (64, 51, 12, 16, None, 16000), (128, 128, 64, 16, 4, 16000), (2048, 1200, 300, 80, 4, 24000)]
    assert all(by[n].win < by[n].n_fft and by[n].n_fft == 64 for n in C.PADDED_WINDOW)
    assert by["odd_window_hop12_unit"].win % 2 == 1 and by["odd_window_hop12_unit"].n_fft % by["odd_window_hop12_unit"].hop != 0
    assert by["nfft2048"].n_fft // 4 > 256                       # butterflies per stage > threads of a workgroup
    assert [c.k0 for c in C.CASES] == [3, 3, 2, 4]
    for c in C.CASES:
        assert c.hop < c.win                                      # never hop >= Frame_Length (see audio_cases)
        hp = c.hp()
        assert hp["Sound"] == c.sound and hp["Tacotron2"] == C.hparams.load_hp()["Tacotron2"]


@pytest.mark.parametrize("name", C.NAMES)
def test_every_case_is_accepted_at_create(name):
    """gsttaco_create validates the Sound section on the host: no GPU needed to know that the GPU test will get a context."""
    from gst_tacotron_amd import capi
    capi.Context(C.BY_NAME[name].hp(), max_batch=5, max_tokens=8, max_ref_frames=4, max_wav_seconds=4.0).close()


@pytest.mark.parametrize("top_db", C.TOP_DBS)
@pytest.mark.parametrize("name", C.NAMES)
def test_front_end_batch_has_the_rows_it_claims(name, top_db):
    c = C.BY_NAME[name]
    H = c.n_fft // 2
    full, short, zero, tiny, edge = C.front_batch(name, top_db)
    assert all(w.dtype == np.float32 and w.ndim == 1 for w in (full, short, zero, tiny, edge))
    assert full.shape[0] == 6 * c.n_fft and short.shape[0] < full.shape[0] and zero.shape[0] == 300 and tiny.shape[0] == 17
    assert not zero.any() and C.trimmed(zero, top_db) == (0, 300)              # all frames tie with the maximum: nothing is cut
    frames = [C.expected_frames(c, w, top_db) for w in (full, short, zero, tiny, edge)]
    tl = C.trimmed(edge, top_db)[1]
    print(name, top_db, "frames", frames, "trimmed lengths", [C.trimmed(w, top_db) for w in (full, short, zero, tiny, edge)])
    assert H < tl <= H + 16                                                     # just above what librosa.stft accepts
    assert frames[4] == 1 + tl // c.hop >= 2 and frames[3] == 0
    assert frames[2] == (1 + 300 // c.hop if 300 > H else 0)
    assert 2 <= frames[1] < frames[0] <= 30
    for w in (full, short):                                                     # the trim cuts at both ends
        s, n = C.trimmed(w, top_db)
        assert s > 0 and s + n < w.shape[0]
    if top_db == 15:                                                            # ... and more at 15 dB than at 60
        assert C.trimmed(full, 15)[1] < C.trimmed(C.front_batch(name, 60)[0], 60)[1]
    refs = C.front_reference(name, top_db)
    assert [r is None for r in refs] == [n == 0 for n in frames]
    if refs[2] is not None:
        assert (refs[2] == np.float32(c.mel_floor)).all()                       # silence sits at exactly the floor value


@pytest.mark.parametrize("name", C.NAMES)
def test_front_end_float32_headroom_and_range(name):
    """A float32 evaluation of the front end stays within a quarter of the tolerance of the float64 oracle, on every valid row
    (the edge burst and silence included), and the mels of the two long rows vary over their range instead of sitting on a clip."""
    c = C.BY_NAME[name]
    worst = 0.0
    for top_db in C.TOP_DBS:
        for i, (wav, ref) in enumerate(zip(C.front_batch(name, top_db), C.front_reference(name, top_db))):
            if ref is None:
                continue
            got = C.mel_float32(c, wav, top_db)
            assert got.shape == ref.shape and np.isfinite(ref).all()
            err = float(np.abs(got.astype(np.float64) - ref).max())
            worst = max(worst, err)
            if i < 2:
                inside = float(((ref > c.mel_floor) & (ref < (c.max_abs or 1.0))).mean())
                print(name, top_db, "row", i, "mel range", float(ref.min()), float(ref.max()), "fraction off the clips", inside)
                assert inside >= 0.5 and float(np.ptp(ref)) >= 0.3 * (2 * c.max_abs if c.max_abs else 1.0)
    print(name, "front end, float32 against the float64 oracle: max abs", worst, "allowed", c.mel_tol / 4)
    assert worst <= c.mel_tol / 4


@pytest.mark.parametrize("name", C.PADDED_WINDOW)
def test_front_end_sees_a_window_one_sample_off_centre(name):
    c = C.BY_NAME[name]
    for shift in (1, -1):
        moved = min(float(np.abs(C.mel_float32(c, wav, 60, window_shift=shift).astype(np.float64) - ref).max())
                    for wav, ref in list(zip(C.front_batch(name, 60), C.front_reference(name, 60)))[:2])
        print(name, "window shifted by", shift, "moves the mels by", moved, "tolerance", c.mel_tol)
        assert moved >= 10 * c.mel_tol


def _gl_rows(c):
    _, frames, _ = C.gl_batch(c.name)
    return [(0, C.GL_FRAMES), (4, int(frames[4]))] + [(r, C.GL_FRAMES) for r in (1, 2, 3, 4)]


@pytest.mark.parametrize("iters", C.GL_ITERS)
@pytest.mark.parametrize("name", C.NAMES)
def test_griffin_lim_float32_headroom(name, iters):
    """Every (row, frame count) the GPU test compares: the float32 restatement stays within a quarter of GL_TOL (relative to the
    oracle's peak) of the oracle, whose waveform is finite and of ordinary size."""
    c = C.BY_NAME[name]
    spec, frames, ph = C.gl_batch(name)
    assert C.GL_FRAMES in range(9, 13) and spec.shape == (5, C.GL_FRAMES, c.nb)
    assert frames.tolist() == [C.GL_FRAMES, 0, 1, c.k0, c.k0 + 1]
    assert float(spec.min()) >= c.mel_floor and float(np.ptp(spec)) >= 0.3 * (2 * c.max_abs if c.max_abs else 1.0)
    worst = 0.0
    for row, T in _gl_rows(c):
        ref = C.gl_reference(name, row, T, iters)
        got = C.inv_spectrogram_float32(c, spec[row, :T], ph[row, :T], iters)
        peak = float(np.abs(ref).max())
        err = float(np.abs(got - ref).max()) / peak
        print(name, "iters", iters, "row", row, "frames", T, "peak", peak, "float32 rel err", err)
        assert np.isfinite(ref).all() and 1e-3 < peak < 10.0
        worst = max(worst, err)
    assert worst <= C.GL_TOL / 4


@pytest.mark.parametrize("iters", C.GL_ITERS)
@pytest.mark.parametrize("name", C.PADDED_WINDOW)
def test_griffin_lim_sees_a_sum_square_from_the_unpadded_position(name, iters):
    c = C.BY_NAME[name]
    spec, _, ph = C.gl_batch(name)
    ref = C.gl_reference(name, 0, C.GL_FRAMES, iters)
    wrong = C.inv_spectrogram_float32(c, spec[0], ph[0], iters, wss_shift=-((c.n_fft - c.win) // 2))
    moved = float(np.abs(wrong - ref).max() / np.abs(ref).max())
    print(name, "iters", iters, "sum-square at the unpadded position moves the waveform by", moved, "of its peak")
    assert moved >= 10 * C.GL_TOL
