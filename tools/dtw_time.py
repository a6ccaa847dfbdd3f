"""What the free-run metric costs beside the synthesis it judges: gsttaco_mel_dtw (csrc/dtw.hip) at 32 x 1000 x 1000 and 128 x 1000 x 1000
frames, n_ceps 13, with and without the path, and an Inference_Step of the same batch (128 tokens, 500 steps = 1000 frames, the headline
configuration) in the same process.  y is a warped copy of x with lengths between 600 and 1000, so the sweep runs 1600 .. 2000
anti-diagonals per utterance.  Every call is timed on its own between two events; the median of CALLS calls after a warm-up of every
form.  A second table splits the alignment launch: lengths of 1 on one side leave the feature kernel and 1000 diagonals of one cell.
python tools/dtw_time.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gst_tacotron_amd import synthetic, weights
from gst_tacotron_amd.model import GST_Tacotron

CALLS = 20
BATCHES, Tv, Tref, STEPS, T = (32, 128), 128, 64, 500, 1000

hp = synthetic.config_hp("cfg2")
assert hp["Max_Step"] == T and hp["Step_Reduction"] * STEPS == T
rng = np.random.default_rng(1)
Bmax = max(BATCHES)
m = GST_Tacotron(hyper_parameters=hp, max_batch=Bmax, max_tokens=Tv, max_ref_frames=Tref + 1)
m.Restore(weights=weights.synthetic_weights(hp, seed=0))
tokens, _ = synthetic.make_tokens(rng, Bmax, Tv)
mels, ml = synthetic.make_ref_mels(rng, Bmax, Tref)
tokens, mels, ml = m._dev(tokens, torch.int32), m._dev(mels, torch.float32), m._dev(ml, torch.int32)

x = np.clip(rng.normal(0.0, 1.5, (Bmax, T, 80)), -4, 4).astype(np.float32)
x_len = rng.integers(600, T + 1, Bmax).astype(np.int32)
y_len = rng.integers(600, T + 1, Bmax).astype(np.int32)
y = np.zeros_like(x)
for b in range(Bmax):
    idx = np.sort(rng.integers(0, x_len[b], y_len[b]))
    y[b, :y_len[b]] = np.clip(x[b, idx] + rng.normal(0.0, 0.05, (y_len[b], 80)), -4, 4)
x, y, x_len, y_len = m._dev(x, torch.float32), m._dev(y, torch.float32), m._dev(x_len, torch.int32), m._dev(y_len, torch.int32)
ones = torch.ones_like(x_len)


def timed(f):
    for i in range(3):
        f(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f(100 + i)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


for B in BATCHES:
    forms = {"Inference_Step (%d steps)" % STEPS: lambda i: m.Inference_Step(tokens[:B], None, None, mels[:B], ml[:B], seed=i, steps=STEPS),
             "mel_dtw, cost only": lambda i: m.Mel_DTW(x[:B], x_len[:B], y[:B], y_len[:B]),
             "mel_dtw, with the path": lambda i: m.Mel_DTW(x[:B], x_len[:B], y[:B], y_len[:B], return_path=True),
             "mel_dtw, y lengths 1 (features + 600..1000 one-cell diagonals)": lambda i: m.Mel_DTW(x[:B], x_len[:B], y[:B], ones[:B]),
             "mel_dtw, both lengths 1 (launches + features of two frames)": lambda i: m.Mel_DTW(x[:B], ones[:B], y[:B], ones[:B])}
    res = {k: timed(f) for k, f in forms.items()}
    step = res["Inference_Step (%d steps)" % STEPS][0]
    cost, n = m.Mel_DTW(x[:B], x_len[:B], y[:B], y_len[:B])
    print("batch %d x %d x %d frames: mean cost / path_len %.3f dB, mean path_len %.0f" % (B, T, T, float((cost / n).mean()), float(n.float().mean())))
    for k, (med, lo, hi) in res.items():
        print("  %-66s median %9.3f ms of %d calls, min %9.3f max %9.3f, %6.3f of the Inference_Step" % (k, med, CALLS, lo, hi, med / step))
m.synchronize()
