"""GPU tests of the device resampler: gsttaco_resample (csrc/resample.hip) straight through the C ABI against the float64 restatement
of tests/resample_cases.py at the derived bound -- every case, a mixed batch, the table cache, back-to-back calls, the refusals -- and
end to end through Mel_Generate.  Output buffers are NaN-filled and longer than needed, so a write outside a row shows."""
import ctypes

import numpy as np
import pytest

import resample_cases as R
from gst_tacotron_amd import audio, hparams

pytestmark = pytest.mark.gpu

I32P = ctypes.POINTER(ctypes.c_int32)
E_INVALID, E_CAPACITY = -1, -5
GUARD = 37          # floats in front of and behind the output, beyond ld_out * B
TARGET = 16000


@pytest.fixture(scope="module")
def model():
    from gst_tacotron_amd.model import GST_Tacotron
    m = GST_Tacotron(hyper_parameters=hparams.load_hp(), max_batch=12, max_tokens=8, max_ref_frames=4, max_wav_seconds=2.0)  # no Restore
    yield m
    m.synchronize()


def _enqueue(m, rows, sr_out, ld_out=None, ld_in=None):
    """rows: [(x, sr_in)].  Enqueues one gsttaco_resample and returns what reads it back later: (rc, device buffer, out_lengths, ld_out).
    The output lies between two guard bands in one NaN-filled buffer."""
    import torch
    B = len(rows)
    in_len = np.array([np.shape(x)[0] for x, _ in rows], dtype=np.int32)
    rates = np.array([r for _, r in rows], dtype=np.int32)
    if ld_in is None:
        ld_in = max(int(in_len.max()), 1) + 3
    if ld_out is None:
        ld_out = max(max(audio.resample_lengths(int(n), int(r), sr_out)[1] for n, r in zip(in_len, rates)), 1) + 5
    host = np.full((B, ld_in), np.nan, dtype=np.float32)        # (samples beyond a row's length must not be read into a result)
    for i, (x, _) in enumerate(rows):
        host[i, :in_len[i]] = x
    xd = torch.from_numpy(host).to(m.device)
    buf = torch.full((GUARD + B * ld_out + GUARD,), float("nan"), dtype=torch.float32, device=m.device)
    out_len = np.full((B,), -7, dtype=np.int32)
    with torch.cuda.device(m.device):
        rc = m.ctx.lib.gsttaco_resample(m.ctx.handle, ctypes.c_void_p(xd.data_ptr()), in_len.ctypes.data_as(I32P), rates.ctypes.data_as(I32P),
                                        B, ld_in, sr_out, ctypes.c_void_p(buf.data_ptr() + 4 * GUARD), ld_out, out_len.ctypes.data_as(I32P),
                                        m._stream())
    return rc, (buf, xd), out_len, ld_out


def _read(pending, B):
    import torch
    rc, (buf, _), out_len, ld_out = pending
    assert rc == 0
    torch.cuda.synchronize()
    flat = buf.cpu().numpy()
    assert np.isnan(flat[:GUARD]).all() and np.isnan(flat[GUARD + B * ld_out:]).all(), "written outside the output"
    return flat[GUARD:GUARD + B * ld_out].reshape(B, ld_out), out_len


def _run(m, rows, sr_out, **kw):
    return _read(_enqueue(m, rows, sr_out, **kw), len(rows))


def _check_row(y, n_fix_got, case, sr_out=None):
    """One output row against the restatement of the case's samples and source rate (to the case's own target, or to ``sr_out``) at
    the derived bound; exact zeros behind it."""
    same = sr_out is None or sr_out == case.sr_out
    y64, _, N, n_fix = case.ref() if same else R.reference(case.x, case.sr_in, sr_out)
    n_out = y64.shape[0]
    assert n_fix_got == n_fix
    got = y[:n_out].astype(np.float64)
    bound = R.gpu_bound(y64, N, case.x)
    err = np.abs(got - y64)
    if n_out:
        print(case.name, "to", sr_out or case.sr_out, "largest |y - ref64| / bound: %.3g" % float((err / np.maximum(bound, 1e-300)).max()))
    assert np.isfinite(got).all() and (err <= bound).all(), (case.name, int(np.argmax(err - bound)))
    tail = y[n_out:]
    assert (tail == 0.0).all() and not np.signbit(tail).any()


@pytest.mark.parametrize("case", R.CASES, ids=R.NAMES)
def test_every_case_is_within_the_derived_bound_of_the_restatement(model, case):
    y, out_len = _run(model, [(case.x, case.sr_in)], case.sr_out)
    _check_row(y[0], int(out_len[0]), case)
    if case.sr_in == case.sr_out:
        assert np.array_equal(y[0, :case.n].view(np.uint32), case.x.view(np.uint32))


def test_a_row_in_a_mixed_batch_is_bitwise_the_row_alone(model):
    """Cases 1, 3, 5, 6 and 12 in one batch.  A call has one target rate, and cases 3 and 6 have targets of their own: their rows go
    in with their samples and source rates (48 kHz, 16 kHz) to the batch's 16 kHz, so case 6's row is a second pass-through.  Every
    row is held to the bound too, against the restatement to 16 kHz."""
    cases = [R.BY_NUMBER[k] for k in (1, 3, 5, 6, 12)]
    rows = [(c.x, c.sr_in) for c in cases]
    y, out_len = _run(model, rows, TARGET)
    ld = y.shape[1]
    for b, (x, sr) in enumerate(rows):
        alone, alone_len = _run(model, [(x, sr)], TARGET, ld_out=ld)
        assert alone_len[0] == out_len[b] == audio.resample_lengths(x.shape[0], sr, TARGET)[1]
        assert np.array_equal(alone[0].view(np.uint32), y[b].view(np.uint32)), cases[b].name
        _check_row(y[b], int(out_len[b]), cases[b], TARGET)
    for b in (3, 4):                            # the pass-through rows: their input, bitwise
        assert np.array_equal(y[b, :cases[b].n].view(np.uint32), cases[b].x.view(np.uint32))


def test_the_table_cache_evicts_and_rebuilds_bitwise(model):
    c = R.BY_NUMBER[2]
    first, _ = _run(model, [(c.x, c.sr_in)], c.sr_out)
    again, _ = _run(model, [(c.x, c.sr_in)], c.sr_out)
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    x = R.BY_NUMBER[9].x
    for k in range(9):                          # nine further pairs: the first one leaves the eight-pair cache
        y, out_len = _run(model, [(x, 30000 + 1000 * k)], c.sr_out)
        n_out, n_fix = audio.resample_lengths(x.shape[0], 30000 + 1000 * k, c.sr_out)
        assert out_len[0] == n_fix and np.isfinite(y[0, :n_out]).all() and (y[0, n_out:] == 0.0).all()
    rebuilt, _ = _run(model, [(c.x, c.sr_in)], c.sr_out)
    assert np.array_equal(first.view(np.uint32), rebuilt.view(np.uint32))


def test_two_calls_back_to_back_on_one_stream_are_both_right(model):
    """Different shapes, rate pairs and row counts, no synchronisation between the calls: the second call's per-row parameters and
    tables must not reach the first call's launch."""
    a_cases = [R.BY_NUMBER[1], R.BY_NUMBER[5]]
    b_cases = [R.BY_NUMBER[9], R.BY_NUMBER[2], R.BY_NUMBER[4]]
    pa = _enqueue(model, [(c.x, c.sr_in) for c in a_cases], TARGET)
    pb = _enqueue(model, [(c.x, c.sr_in) for c in b_cases], TARGET)
    (ya, la), (yb, lb) = _read(pa, 2), _read(pb, 3)
    for y, lens, cases in ((ya, la, a_cases), (yb, lb, b_cases)):
        for b, c in enumerate(cases):
            _check_row(y[b], int(lens[b]), c)


def test_mel_generate_resamples_on_the_device_and_the_host_path_is_todays(model):
    from gst_tacotron_amd.model import GST_Tacotron
    c = R.BY_NUMBER[13]
    y, lens = model.Resample([c.x], 22050)
    assert lens.dtype == np.int32 and lens.tolist() == [24000] and tuple(y.shape) == (1, 24000)
    _check_row(y[0].cpu().numpy(), int(lens[0]), c)
    mels, mel_len = model.Mel_Generate([(c.x, 22050)])
    mels2, mel_len2 = model.Mel_Generate([y[0, :lens[0]].cpu().numpy()])
    assert np.array_equal(mels.cpu().numpy().view(np.uint32), mels2.cpu().numpy().view(np.uint32))
    assert np.array_equal(mel_len.cpu().numpy(), mel_len2.cpu().numpy()) and int(mel_len[0]) > 50
    feats = model.Feature_Generate([(c.x, 22050)])
    assert np.array_equal(feats[0].cpu().numpy().view(np.uint32), mels.cpu().numpy().view(np.uint32))
    host = GST_Tacotron(hyper_parameters=hparams.load_hp(), max_batch=2, max_tokens=8, max_ref_frames=4, max_wav_seconds=2.0, resample="host")
    mh, lh = host.Mel_Generate([(c.x, 22050)])
    mt, lt = host.Mel_Generate([audio.resample_kaiser_best(c.x, 22050, TARGET)])
    assert np.array_equal(mh.cpu().numpy().view(np.uint32), mt.cpu().numpy().view(np.uint32))
    assert np.array_equal(lh.cpu().numpy(), lt.cpu().numpy())
    host.synchronize()


def test_refusals_return_their_code_and_leave_the_output_untouched(model):
    import torch
    x = R.BY_NUMBER[9].x
    cap = model.ctx.cfg.max_wav_samples

    def refused(pending, code, B=1):
        rc, (buf, _), out_len, _ = pending
        assert rc == code, (rc, model.last_message())
        torch.cuda.synchronize()
        assert np.isnan(buf.cpu().numpy()).all() and (out_len == -7).all()
        return model.ctx.lib.gsttaco_last_error(model.ctx.handle).decode()

    refused(_enqueue(model, [(x, 16 * TARGET + 1)], TARGET), E_INVALID)           # down by more than 16
    refused(_enqueue(model, [(x, 999)], TARGET), E_INVALID)                       # up by more than 16
    refused(_enqueue(model, [(x, 22050)], TARGET, ld_out=cap + 1), E_CAPACITY)
    n_fix = audio.resample_lengths(x.shape[0], 22050, TARGET)[1]
    refused(_enqueue(model, [(x, 22050)], TARGET, ld_out=n_fix - 1), E_INVALID)   # a row longer than ld_out
    msg = refused(_enqueue(model, [(x[:8], 20000 + 100 * k) for k in range(9)], TARGET), E_INVALID, B=9)         # nine distinct pairs
    assert "eight" in msg
    # ... while nine rows of eight pairs and a pass-through are one call
    y, out_len = _run(model, [(x[:8], 20000 + 100 * (k % 8)) for k in range(9)] + [(x[:8], TARGET)], TARGET)
    assert np.array_equal(y[0].view(np.uint32), y[8].view(np.uint32)) and np.array_equal(y[9, :8], x[:8])
    # a null pointer, for each of the five
    good = _enqueue(model, [(x, 22050)], TARGET)
    _read(good, 1)
    _, (buf, xd), out_len, ld_out = good
    keep = buf.cpu().numpy().copy()
    n_in, rate = np.array([x.shape[0]], dtype=np.int32), np.array([22050], dtype=np.int32)
    args = [ctypes.c_void_p(xd.data_ptr()), n_in.ctypes.data_as(I32P), rate.ctypes.data_as(I32P), 1, xd.shape[1], TARGET,
            ctypes.c_void_p(buf.data_ptr() + 4 * GUARD), ld_out, out_len.ctypes.data_as(I32P), model._stream()]
    for k in (0, 1, 2, 6, 8):
        a = list(args)
        a[k] = None
        out_len[:] = -7
        with torch.cuda.device(model.device):
            assert model.ctx.lib.gsttaco_resample(model.ctx.handle, *a) == E_INVALID
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), keep.view(np.uint32)) and (out_len == -7).all()
