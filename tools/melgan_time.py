"""What the neural vocoder costs beside the synthesis it voices: gsttaco_melgan (csrc/melgan.hip) at the default sizes on 1 x 200,
32 x 1000 and 128 x 1000 frames -- the whole call, and every launch of it alone (gsttaco_melgan_debug_stage) with its multiply-adds
and the share of the fp32 MFMA peak (157.3 TFLOP/s) they amount to -- beside the 60 Griffin-Lim iterations (Inv_Spectrogram) and the
Inference_Step (128 tokens, the headline configuration, steps = frames / 2) of the same batch in the same process.  Every call is
timed on its own between two events: ROUNDS rounds of CALLS calls after a warm-up of every form, the median of all calls and the
spread of the rounds' medians.
python tools/melgan_time.py"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from gst_tacotron_amd import melgan, synthetic, weights
from gst_tacotron_amd.model import GST_Tacotron, _ptr

ROUNDS, CALLS = 3, 5
SHAPES, Tv, Tref = ((1, 200), (32, 1000), (128, 1000)), 128, 64
PEAK = 157.3e12

hp = synthetic.config_hp("cfg2")
hop = hp["Sound"]["Frame_Shift"]
Bmax, Tmax = max(b for b, _ in SHAPES), max(t for _, t in SHAPES)
rng = np.random.default_rng(1)
m = GST_Tacotron(hyper_parameters=hp, max_batch=Bmax, max_tokens=Tv, max_ref_frames=Tref + 1, max_wav_seconds=hop * Tmax / hp["Sound"]["Sample_Rate"] + 1)
m.Restore(weights=weights.synthetic_weights(hp, seed=0))
cfg = melgan.MelGANConfig()
m.Load_Neural_Vocoder(melgan.synthetic_weights(cfg, seed=0), max_frames=Tmax)
min_frames, _, stages = m.ctx.melgan_plan()
tokens, _ = synthetic.make_tokens(rng, Bmax, Tv)
ref, ml = synthetic.make_ref_mels(rng, Bmax, Tref)
tokens, ref, ml = m._dev(tokens, torch.int32), m._dev(ref, torch.float32), m._dev(ml, torch.int32)
mel = m._dev(np.clip(rng.normal(0.0, 1.5, (Bmax, Tmax, 80)), -4, 4).astype(np.float32), torch.float32)
spec = torch.rand((Bmax, Tmax, hp["Sound"]["Spectrogram_Dim"]), device=m.device) * 8 - 4

# multiply-adds per mel frame of each launch
ch, macs, rate = cfg.channels(), [7 * cfg.mel_dim * cfg.channels()[0]], 1
for i, r in enumerate(cfg.ratios):
    rate *= r
    macs.append(2 * ch[i] * ch[i + 1] * rate)
    macs += [5 * ch[i + 1] * ch[i + 1] * rate] * cfg.n_res
macs.append(7 * cfg.base * rate)
assert len(macs) == len(stages)


def timed(f):
    for i in range(2):
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


for B, T in SHAPES:
    x = mel[:B, :T].contiguous()
    sp = spec[:B, :T].contiguous()
    frames = m._dev(np.full(B, T, np.int32), torch.int32)
    wav = torch.empty((B, T * hop), dtype=torch.float32, device=m.device)

    def stage(k):
        m.ctx.check(m.ctx.lib.gsttaco_melgan_debug_stage(m.ctx.handle, k, _ptr(x), None, B, T, _ptr(wav), T * hop, m._stream()))

    forms = {"Inference_Step (%d steps)" % (T // 2): lambda i: m.Inference_Step(tokens[:B], None, None, ref[:B], ml[:B], seed=i, steps=T // 2),
             "Inv_Spectrogram (60 iterations)": lambda i: m.Inv_Spectrogram(sp, frames=frames, seed=i),
             "Neural_Vocoder": lambda i: m.Neural_Vocoder(x)}
    res = {}
    for k, f in forms.items():
        try:
            res[k] = timed(f)
        except Exception as e:                   # (a batch the decode's capacity does not take: the other figures still stand)
            print("  %s: not run (%s)" % (k, str(e)[:100]))
    voc = res["Neural_Vocoder"][0]
    print("batch %d x %d frames: %.1f M multiply-adds a frame, %.2f TFLOP a call, %.1f TFLOP/s = %.3f of the fp32 MFMA peak, %.2f M frames/s"
          % (B, T, sum(macs) / 1e6, 2 * sum(macs) * B * T / 1e12, 2 * sum(macs) * B * T / voc / 1e9, 2 * sum(macs) * B * T / voc / 1e-3 / PEAK,
             B * T / voc / 1e3))
    for k, (med, lo, hi) in res.items():
        print("  %-34s median %10.3f ms of %d x %d calls, round medians %10.3f .. %10.3f, %7.3f of the Neural_Vocoder" %
              (k, med, ROUNDS, CALLS, lo, hi, med / voc))
    m.Neural_Vocoder(x)                         # the workspace now holds this shape's activations
    total = 0.0
    for k, s in enumerate(stages):
        med, lo, hi = timed(lambda i: stage(k))
        total += med
        print("    launch %2d %-3s %4d ch, tile %3d, form %d: %9.3f ms (%9.3f .. %9.3f), %7.1f M multiply-adds a frame, %.3f of the peak"
              % (k, s["kind"], s["channels"], s["tile"], s["form"], med, lo, hi, macs[k] / 1e6, 2 * macs[k] * B * T / (med * 1e-3) / PEAK))
    print("    sum of the launches %.3f ms" % total)
m.synchronize()
