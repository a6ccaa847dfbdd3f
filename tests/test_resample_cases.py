"""Admits the case table of tests/resample_cases.py with no GPU: the float64 restatement the device resampler is held to agrees with
the product's host function and with the oracle's loop-for-loop restatement of resampy, the register cases do tell an accumulated
time register from an exact one, and the host-side surface (lengths, read_wav / load_wav, the ABI) is what the device path relies on."""
import os
import re
import wave

import numpy as np
import pytest

import resample_cases as R
from gst_tacotron_amd import audio, capi
from oracle import audio_np as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", R.CASES, ids=R.NAMES)
def test_restatement_is_within_one_float32_ulp_of_the_host_function(case):
    """Both sum the same float64 terms (the host function pairwise, the restatement in tap order): 1e-16 apart before the one
    rounding to float32, so at most neighbouring floats after it."""
    want = audio.as_signal((case.x, case.sr_in), case.sr_out)
    got = case.padded()
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()


@pytest.mark.parametrize("case", [c for c in R.CASES if c.sr_in != c.sr_out], ids=[c.name for c in R.CASES if c.sr_in != c.sr_out])
def test_restatement_is_within_the_per_tap_rounding_of_the_oracle(case):
    """oracle/audio_np.py rounds the accumulator to float32 after every tap as resampy does: N roundings of at most 2^-24 of a
    partial sum that A bounds.  64-sample slices (the oracle is a Python loop): the start, the middle and the end."""
    y64, Aabs, N, _ = case.ref()
    n_out = y64.shape[0]
    starts = sorted({0, max(0, n_out // 2 - 32), max(0, n_out - 64)})
    for t0 in starts:
        t1 = min(t0 + 64, n_out)
        got = A.resample_kaiser_best(case.x, case.sr_in, case.sr_out, t0, t1)
        assert got.shape == (t1 - t0,)
        bound = N[t0:t1] * 2.0 ** -24 * Aabs[t0:t1]
        assert (np.abs(got.astype(np.float64) - y64[t0:t1]) <= bound).all(), (case.name, t0)


def test_restatement_is_within_the_per_tap_rounding_of_the_lj_fixture():
    """The committed output of the oracle's restatement on the LJ excerpt, in full."""
    case = R.BY_NUMBER[13]
    want = np.load(R.GOLDEN_LJ)["resampled"]
    y64, Aabs, N, n_fix = case.ref()
    assert want.shape == (n_fix,) == y64.shape
    assert (np.abs(want.astype(np.float64) - y64) <= N * 2.0 ** -24 * Aabs).all()


@pytest.mark.parametrize("number", R.REGISTER_CASES)
def test_register_cases_tell_the_accumulated_register_from_the_exact_one(number):
    """Each holds an output where the same restatement under exact rational time lands more than 100 times the GPU bound away."""
    case = R.BY_NUMBER[number]
    y_acc, _, N, _ = case.ref()
    y_rat = case.ref("rational")[0]
    n_acc = R.register(y_acc.shape[0], case.sr_in, case.sr_out)[0]
    n_rat = R.register(y_acc.shape[0], case.sr_in, case.sr_out, "rational")[0]
    assert (n_acc != n_rat).any()
    excess = np.abs(y_acc - y_rat) / R.gpu_bound(y_acc, N, case.x)
    print(case.name, "outputs whose registers differ:", np.flatnonzero(n_acc != n_rat)[:8], "largest distance / bound:", excess.max(),
          "distance:", np.abs(y_acc - y_rat).max())
    assert excess.max() > 100.0


def test_resample_lengths_equal_the_products_lengths():
    for sr_in, sr_out in [(22050, 16000), (44100, 16000), (48000, 16000), (8000, 16000), (16000, 24000), (16001, 16000), (48000, 22050),
                          (256000, 16000), (1000, 16000)]:
        for n in list(range(0, 40)) + [147, 441, 997]:
            n_out, n_fix = audio.resample_lengths(n, sr_in, sr_out)
            y = audio.resample_kaiser_best(np.zeros(n, dtype=np.float32), sr_in, sr_out)
            ratio = float(sr_out) / float(sr_in)
            assert y.shape == (n_fix,) and n_out == int(n * ratio) and 0 <= n_fix - n_out <= 1


def test_load_wav_is_read_wav_then_the_resampling(tmp_path):
    p = str(tmp_path / "a.wav")
    pcm = (np.random.default_rng(3).uniform(-0.5, 0.5, (500, 2)) * 32767).astype("<i2")
    with wave.open(p, "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(8000)
        f.writeframes(pcm.tobytes())
    x, sr = audio.read_wav(p)
    assert sr == 8000 and x.dtype == np.float32 and x.shape == (500,)
    assert np.array_equal(x, (pcm.astype(np.float32) / 32768.0).mean(axis=1).astype(np.float32))
    y = audio.load_wav(p, 16000)
    assert y.shape == (1000,) and np.array_equal(y, audio.resample_kaiser_best(x, sr, 16000))
    assert np.array_equal(audio.load_wav(p, 8000), x)
    # the three spellings of a reference signal
    for item, want in ((p, (x, 8000)), ((x, 8000), (x, 8000)), (x, (x, 16000))):
        s, r = audio.as_signal_at_rate(item, 16000)
        assert r == want[1] and np.array_equal(s, want[0])
    assert np.array_equal(audio.as_signal((x, 8000), 16000), y) and np.array_equal(audio.as_signal(p, 16000), y)


def test_abi_surface_of_the_resampler():
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    m = re.search(r"\bint gsttaco_resample\(([^;]*)\);", header)
    assert m, "include/gsttaco.h does not declare int gsttaco_resample("
    n_args = len(m.group(1).split(","))
    assert n_args == 11
    assert "gsttaco_resample" in capi.EXPORTED_SYMBOLS
    assert capi.ABI_VERSION == 14 and re.search(r"#define\s+GSTTACO_ABI_VERSION\s+14\b", header)
    lib = capi.load_library()
    assert len(lib.gsttaco_resample.argtypes) == n_args and lib.gsttaco_resample.restype is not None
