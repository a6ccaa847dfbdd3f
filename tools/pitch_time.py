"""What the prosody metrics cost beside the synthesis they judge: gsttaco_pitch (csrc/pitch.hip) at the default settings (50..500 Hz, 321
lags, W = 400) on 32 and 128 rows x 5 s, with and without the trim, and gsttaco_pitch_errors on 1000 x 1000-frame paths, beside the
Inv_Spectrogram and the Inference_Step (128 tokens, 500 steps = 1000 frames, the headline configuration) of the same batch in the same
process, and beside the NumPy restatement of tests/pitch_cases.py on the host (one row of 1 s timed, multiplied out).  The rows are
harmonic complexes with a gliding fundamental between noise, so voiced and unvoiced frames both occur.  Every call is timed on its own
between two events: ROUNDS rounds of CALLS calls after a warm-up of every form, the median of all calls and the spread of the rounds'
medians.
python tools/pitch_time.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from gst_tacotron_amd import synthetic, weights
from gst_tacotron_amd.model import GST_Tacotron

ROUNDS, CALLS = 5, 10
BATCHES, Tv, Tref, STEPS, T, SECONDS = (32, 128), 128, 64, 500, 1000, 5.0

hp = synthetic.config_hp("cfg2")
assert hp["Max_Step"] == T and hp["Step_Reduction"] * STEPS == T
sr, hop = hp["Sound"]["Sample_Rate"], hp["Sound"]["Frame_Shift"]
rng = np.random.default_rng(1)
Bmax = max(BATCHES)
m = GST_Tacotron(hyper_parameters=hp, max_batch=Bmax, max_tokens=Tv, max_ref_frames=Tref + 1, max_wav_seconds=max(SECONDS, hop * T / sr) + 1)
m.Restore(weights=weights.synthetic_weights(hp, seed=0))
tokens, _ = synthetic.make_tokens(rng, Bmax, Tv)
mels, ml = synthetic.make_ref_mels(rng, Bmax, Tref)
tokens, mels, ml = m._dev(tokens, torch.int32), m._dev(mels, torch.float32), m._dev(ml, torch.int32)

n = int(SECONDS * sr)
t = np.arange(n) / sr
wav = np.zeros((Bmax, n), np.float32)
for b in range(Bmax):
    f = rng.uniform(90, 250) * (1 + 0.2 * np.sin(2 * np.pi * rng.uniform(0.3, 1.0) * t))
    ph = 2 * np.pi * np.cumsum(f) / sr
    voiced = (np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * t + rng.uniform(0, 6)) > -0.3)
    wav[b] = np.where(voiced, 0.2 * np.sin(ph) + 0.1 * np.sin(2 * ph) + 0.05 * np.sin(3 * ph), 0) + 0.01 * rng.standard_normal(n)
wav_d = m._dev(wav, torch.float32)
len_d = m._dev(np.full(Bmax, n, np.int32), torch.int32)

fx = np.where(rng.random((Bmax, T)) < 0.3, 0, rng.uniform(80, 300, (Bmax, T))).astype(np.float32)
fy = np.where(rng.random((Bmax, T)) < 0.3, 0, rng.uniform(80, 300, (Bmax, T))).astype(np.float32)
x = np.clip(rng.normal(0.0, 1.5, (Bmax, T, 80)), -4, 4).astype(np.float32)
x_len = rng.integers(600, T + 1, Bmax).astype(np.int32)
y_len = rng.integers(600, T + 1, Bmax).astype(np.int32)
y = np.zeros_like(x)
for b in range(Bmax):
    idx = np.sort(rng.integers(0, x_len[b], y_len[b]))
    y[b, :y_len[b]] = np.clip(x[b, idx] + rng.normal(0.0, 0.05, (y_len[b], 80)), -4, 4)
fx, fy, x, y, x_len, y_len = (m._dev(a, dt) for a, dt in ((fx, torch.float32), (fy, torch.float32), (x, torch.float32), (y, torch.float32),
                                                          (x_len, torch.int32), (y_len, torch.int32)))
_, plen, path = m.Mel_DTW(x, x_len, y, y_len, return_path=True)
spec = torch.rand((Bmax, T, hp["Sound"]["Spectrogram_Dim"]), device=m.device) * 8 - 4
frames = m._dev(np.full(Bmax, T, np.int32), torch.int32)


def timed(f):
    for i in range(3):
        f(i)
    torch.cuda.synchronize()
    rounds = []
    for r in range(ROUNDS):
        ms = []
        for i in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(100 + r * CALLS + i)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        rounds.append(ms)
    med = [float(np.median(r)) for r in rounds]
    return float(np.median(np.concatenate(rounds))), min(med), max(med)


for B in BATCHES:
    step_name = "Inference_Step (%d steps)" % STEPS
    forms = {step_name: lambda i: m.Inference_Step(tokens[:B], None, None, mels[:B], ml[:B], seed=i, steps=STEPS),
             "Inv_Spectrogram (%d frames, 60 iterations)" % T: lambda i: m.Inv_Spectrogram(spec[:B], frames=frames[:B], seed=i),
             "pitch, no trim (%.0f s rows)" % SECONDS: lambda i: m.Pitch_Signals(wav_d[:B], len_d[:B]),
             "pitch, top_db 15": lambda i: m.Pitch_Signals(wav_d[:B], len_d[:B], 15),
             "pitch_errors along the DTW path": lambda i: m.Pitch_Errors(fx[:B], x_len[:B], fy[:B], y_len[:B], path[:B], plen[:B]),
             "pitch_errors on the diagonal": lambda i: m.Pitch_Errors(fx[:B], x_len[:B], fy[:B], y_len[:B])}
    res = {k: timed(f) for k, f in forms.items()}
    step = res[step_name][0]
    f0, _, nfr = m.Pitch_Signals(wav_d[:B], len_d[:B])
    print("batch %d: %d frames a row, %.2f of them voiced" % (B, int(nfr[0]), float((f0 > 0).float().mean())))
    for k, (med, lo, hi) in res.items():
        print("  %-46s median %9.3f ms of %d x %d calls, round medians %9.3f .. %9.3f, %6.3f of the Inference_Step" %
              (k, med, ROUNDS, CALLS, lo, hi, med / step))
m.synchronize()

import audio_cases as C
import pitch_cases as P
case = C.Case("timed", hp["Sound"]["Spectrogram_Dim"], hp["Sound"]["Frame_Length"], hop, hp["Sound"]["Mel_Dim"], 4, sample_rate=sr)
t0 = time.perf_counter()
ref = P.pitch_reference(wav[0, :sr], case)
dt = time.perf_counter() - t0
got = m.Pitch([wav[0, :sr]])[0].cpu().numpy()[0]
print("NumPy restatement on the host: %.2f s for one row of 1 s (%d frames) -> %.0f s for 32 rows x %.0f s; device f0 of that row within %.1e relative"
      % (dt, ref["frames"], dt * 32 * SECONDS, SECONDS, float(np.max(np.abs(got[:ref["frames"]] - ref["f0"]) / np.maximum(ref["f0"], 1)))))
