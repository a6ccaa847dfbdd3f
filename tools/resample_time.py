"""What bringing reference audio to Sound.Sample_Rate costs, on the device and on the host: gsttaco_resample (csrc/resample.hip) at
32 rows x 5 s for 22 050, 44 100, 48 000 and 8 000 Hz to 16 000 Hz, the host function audio.resample_kaiser_best on the same inputs on
the same box (the path it replaces: the baseline), gsttaco_mel_frontend at the same batch of 5 s rows at 16 kHz (the kernel this feeds:
the yardstick), and the first call of a new rate pair (the host builds the pair's time register and table and uploads them) apart
from the calls that find it cached.  Every device call is timed on its own between two events with inputs already on the device; the
median of CALLS calls after a warm-up.  The host function is timed on one row (it is a loop over rows) and multiplied out.
python tools/resample_time.py"""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gst_tacotron_amd import audio, hparams
from gst_tacotron_amd.model import GST_Tacotron, _ptr

CALLS, B, SECONDS, TARGET = 20, 32, 5.0, 16000
RATES = (22050, 44100, 48000, 8000)
I32P = ctypes.POINTER(ctypes.c_int32)

m = GST_Tacotron(hyper_parameters=hparams.load_hp(), max_batch=B, max_tokens=8, max_ref_frames=4, max_wav_seconds=SECONDS + 0.5)
rng = np.random.default_rng(1)
audio.resample_kaiser_best(np.zeros(64, dtype=np.float32), 22050, TARGET)       # (the host function's table is built once per process: not timed)


def event_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(f):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ms = [event_ms(f) for _ in range(CALLS)]
    return float(np.median(ms)), min(ms), max(ms)


def resample_call(x, n, rate, y, out_len):
    in_len, rates = np.full((B,), n, dtype=np.int32), np.full((B,), rate, dtype=np.int32)

    def call():
        m.ctx.check(m.ctx.lib.gsttaco_resample(m.ctx.handle, _ptr(x), in_len.ctypes.data_as(I32P), rates.ctypes.data_as(I32P), B, n, TARGET,
                                               _ptr(y), y.shape[1], out_len.ctypes.data_as(I32P), m._stream()))
    return call


n16 = int(SECONDS * TARGET)
wav16 = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, n16)).astype(np.float32)).to(m.device)
len16 = torch.full((B,), n16, dtype=torch.int32, device=m.device)
cap = 2 + n16 // m.dims.frame_shift
mels = torch.empty((B, cap, m.dims.mel), dtype=torch.float32, device=m.device)
mel_len = torch.empty((B,), dtype=torch.int32, device=m.device)
front = timed(lambda: m.ctx.check(m.ctx.lib.gsttaco_mel_frontend(m.ctx.handle, _ptr(wav16), _ptr(len16), B, n16, ctypes.c_float(60.0), _ptr(mels),
                                                                  _ptr(mel_len), cap, m._stream())))
print("gsttaco_mel_frontend, %d rows x %.0f s at %d Hz: median %.3f ms of %d calls, min %.3f max %.3f" % ((B, SECONDS, TARGET, front[0], CALLS) + front[1:]))

for rate in RATES:
    n = int(SECONDS * rate)
    host_x = rng.uniform(-0.5, 0.5, (B, n)).astype(np.float32)
    x = torch.from_numpy(host_x).to(m.device)
    y = torch.empty((B, audio.resample_lengths(n, rate, TARGET)[1]), dtype=torch.float32, device=m.device)
    out_len = np.zeros((B,), dtype=np.int32)
    call = resample_call(x, n, rate, y, out_len)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first_ms = event_ms(call)                   # the pair's first call: register + table on the host, two uploads, the launch
    first_wall = (time.perf_counter() - t0) * 1e3
    med, lo, hi = timed(call)
    t0 = time.perf_counter()
    want = audio.resample_kaiser_best(host_x[0], rate, TARGET)
    host_row = time.perf_counter() - t0
    got = y[0].cpu().numpy()
    apart = int((np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(got), np.abs(want)))).max())
    print("%6d -> %d Hz, %d rows x %.0f s: device median %.3f ms of %d calls, min %.3f max %.3f (%.2f of the front end); first call of the pair "
          "%.3f ms between events, %.3f ms wall; host function %.3f s a row, %.1f s the batch (%.0f times the device call); row 0 at most %d "
          "float32 steps from the host function's" % (rate, TARGET, B, SECONDS, med, CALLS, lo, hi, med / front[0], first_ms, first_wall,
                                                      host_row, host_row * B, host_row * B * 1e3 / med, apart))
m.synchronize()
