"""GPU: the audio kernels (csrc/audio.hip: wav -> mels_for_gst front end, Griffin-Lim back end) against the float64 oracle at the
Sound sections no other test runs -- a zero-padded and an odd window, a hop that does not divide n_fft, the [0, 1] normalisation,
half overlap, n_fft 2048 -- and at the documented length edges.  The cases and their shared references live in tests/audio_cases.py;
tests/test_audio_cases.py shows on the CPU that float32 arithmetic has a factor 4 of room under every tolerance used here and that
a window or a window sum-square at the wrong offset moves the result by >= 10 x the tolerance.

The C entry points are called directly where a row may come back with length 0 (Mel_Generate raises there), with output buffers
longer than needed and pre-filled with NaN, so that an element the kernels never wrote is visible.
"""
import ctypes

import numpy as np
import pytest

import audio_cases as C
from oracle import rng_np

pytestmark = pytest.mark.gpu


def _model(case, B=5):
    from gst_tacotron_amd.model import GST_Tacotron
    return GST_Tacotron(hyper_parameters=case.hp(), max_batch=B, max_tokens=8, max_ref_frames=4, max_wav_seconds=4.0)   # no Restore: no weights here


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _front_end(m, case, wavs, top_db, extra_frames=3):
    """gsttaco_mel_frontend as GST_Tacotron.Mel_Generate calls it -> (mels [B, cap_frames, Mel_Dim], mel_lengths [B]) as NumPy."""
    import torch
    B, ld = len(wavs), max(17, max(w.shape[0] for w in wavs))
    host = np.zeros((B, ld), np.float32)
    for i, w in enumerate(wavs):
        host[i, :w.shape[0]] = w
    wav = torch.from_numpy(host).to(m.device)
    lens = torch.tensor([w.shape[0] for w in wavs], dtype=torch.int32, device=m.device)
    cap = 2 + ld // case.hop + extra_frames
    mels = torch.full((B, cap, case.mel), float("nan"), dtype=torch.float32, device=m.device)
    mel_len = torch.full((B,), -7, dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        m.ctx.check(m.ctx.lib.gsttaco_mel_frontend(m.ctx.handle, _ptr(wav), _ptr(lens), B, ld, ctypes.c_float(float(top_db)),
                                                   _ptr(mels), _ptr(mel_len), cap, m._stream()))
    torch.cuda.synchronize()
    return mels.cpu().numpy(), mel_len.cpu().numpy()


@pytest.mark.parametrize("top_db", C.TOP_DBS)
@pytest.mark.parametrize("name", C.NAMES)
def test_front_end_matches_oracle_at_untested_sections_and_length_edges(name, top_db):
    """One batch of five rows -- full length, shorter, 300 zeros, 17 samples, a burst whose trimmed length is just above n_fft / 2 --
    per Sound section and top_db.  Frame counts are exact (0 where the reference raises), mels within the tolerance (MEL_TOL on the
    [-4, 4] scale, MEL_TOL / 8 on [0, 1]), silence at exactly the floor value, frame 0 and all padding exactly 0 up to cap_frames,
    and every valid row bitwise the row run alone."""
    case = C.BY_NAME[name]
    wavs, refs = C.front_batch(name, top_db), C.front_reference(name, top_db)
    m = _model(case)
    mels, lens = _front_end(m, case, wavs, top_db)
    assert not np.isnan(mels).any(), "an element of the output buffer was never written"
    assert lens.tolist() == [0 if r is None else r.shape[0] for r in refs]
    assert lens[3] == 0                                                          # 17 samples
    assert (mels[:, 0] == 0.0).all()                                             # prepended zero frame (Feeder.py:219-223)
    worst = 0.0
    for i, ref in enumerate(refs):
        n = int(lens[i])
        assert (mels[i, 1 + n:] == 0.0).all(), ("padding of row", i)
        if ref is None:
            continue
        err = float(np.abs(mels[i, 1:1 + n].astype(np.float64) - ref).max())
        print(name, "top_db", top_db, "row", i, "frames", n, "max abs err", err, "tolerance", case.mel_tol)
        worst = max(worst, err)
        if i == 2:
            assert (mels[i, 1:1 + n] == np.float32(case.mel_floor)).all(), "silence is not at the floor value"
        alone, alone_len = _front_end(m, case, [wavs[i]], top_db)
        assert int(alone_len[0]) == n and not np.isnan(alone).any()
        assert np.array_equal(alone[0, :1 + n], mels[i, :1 + n]), ("row", i, "differs from the same wav run alone")
    assert worst <= case.mel_tol


def _griffin_lim(m, case, spec, frames, ph, iters, seed=0, extra=5):
    """gsttaco_griffin_lim as GST_Tacotron.Inv_Spectrogram calls it, at GL_POWER / GL_REF_DB -> (wav [B, ld_wav], wav_lengths [B])."""
    import torch
    B, T = spec.shape[0], spec.shape[1]
    ld = case.hop * (T - 1) + extra
    sp = torch.from_numpy(np.array(spec)).to(m.device)
    fr = None if frames is None else torch.from_numpy(np.array(frames, np.int32)).to(m.device)
    p = None if ph is None else torch.from_numpy(np.array(ph)).to(m.device)
    wav = torch.full((B, ld), float("nan"), dtype=torch.float32, device=m.device)
    lens = torch.full((B,), -7, dtype=torch.int32, device=m.device)
    null = ctypes.c_void_p(None)
    with torch.cuda.device(m.device):
        m.ctx.check(m.ctx.lib.gsttaco_griffin_lim(m.ctx.handle, _ptr(sp), null if fr is None else _ptr(fr), B, T, int(iters),
                                                  ctypes.c_float(C.GL_POWER), ctypes.c_float(C.GL_REF_DB), null if p is None else _ptr(p),
                                                  ctypes.c_uint64(seed), _ptr(wav), _ptr(lens), ld, m._stream()))
    torch.cuda.synchronize()
    return wav.cpu().numpy(), lens.cpu().numpy()


@pytest.mark.parametrize("iters", C.GL_ITERS)
@pytest.mark.parametrize("name", C.NAMES)
def test_griffin_lim_matches_oracle_at_untested_sections_and_frame_edges(name, iters):
    """frames = [T, 0, 1, k0, k0 + 1] with k0 the largest count whose signal librosa.stft cannot pad: rows 1-3 come back empty and
    all zero (the header's contract; the NumPy oracle happens not to raise there and is not compared), rows 0 and 4 match the oracle
    within 2e-3 of its peak at power 1.2 / ref_level_db 15, everything past a row's length is 0 up to ld_wav.  Then frames = NULL:
    every row on all T frames."""
    case = C.BY_NAME[name]
    spec, frames, ph = C.gl_batch(name)
    T = C.GL_FRAMES
    m = _model(case)
    wav, lens = _griffin_lim(m, case, spec, frames, ph, iters)
    assert not np.isnan(wav).any(), "an element of the output buffer was never written"
    assert lens.tolist() == [case.hop * (T - 1), 0, 0, 0, case.hop * case.k0]
    assert (wav[1:4] == 0.0).all()
    for row, n in ((0, T), (4, case.k0 + 1)):
        ref = C.gl_reference(name, row, n, iters)
        L = int(lens[row])
        err = float(np.abs(wav[row, :L] - ref).max() / np.abs(ref).max())
        print(name, "iters", iters, "row", row, "frames", n, "rel err", err)
        assert err <= C.GL_TOL
        assert (wav[row, L:] == 0.0).all()
    wav, lens = _griffin_lim(m, case, spec, None, ph, iters)
    assert not np.isnan(wav).any() and lens.tolist() == [case.hop * (T - 1)] * 5
    for row in range(5):
        ref = C.gl_reference(name, row, T, iters)
        err = float(np.abs(wav[row, :lens[row]] - ref).max() / np.abs(ref).max())
        print(name, "iters", iters, "frames NULL, row", row, "rel err", err)
        assert err <= C.GL_TOL
        assert (wav[row, lens[row]:] == 0.0).all()


@pytest.mark.parametrize("name", ["short_window", "nfft2048"])
def test_griffin_lim_seeded_phases_are_the_host_restatement_bitwise(name):
    """Inv_Spectrogram(seed=S) draws u = (x >> 8) * 2^-24 of Philox counter ((b T + t) bins + k, 0, 0, 0x4000); injecting
    rng_np.gl_phase(S) feeds the kernel the same float32 u, so the two waveforms are bitwise equal -- and the seed's high word counts."""
    import torch
    case = C.BY_NAME[name]
    spec, _, _ = C.gl_batch(name)
    B, T, nb = spec.shape
    m = _model(case)
    S = C.SEED64
    seeded, lens = m.Inv_Spectrogram(np.array(spec), iters=2, seed=S)
    injected, _ = m.Inv_Spectrogram(np.array(spec), iters=2, init_phase=rng_np.gl_phase(S, B, T, nb))
    low, _ = m.Inv_Spectrogram(np.array(spec), iters=2, seed=S & 0xFFFFFFFF)
    torch.cuda.synchronize()
    seeded, injected, low = seeded.cpu().numpy(), injected.cpu().numpy(), low.cpu().numpy()
    assert lens.cpu().numpy().tolist() == [case.hop * (T - 1)] * B and np.isfinite(seeded).all() and np.abs(seeded).max() > 1e-3
    diff = float(np.abs(seeded - injected).max())
    print(name, "seeded vs injected host phases: max abs difference", diff, "; vs the seed's low word alone:", float(np.abs(seeded - low).max()))
    assert np.array_equal(seeded, injected)
    assert not np.array_equal(seeded, low)
