"""What the HiFi-GAN vocoder costs beside the other ways to a waveform: gsttaco_hifigan (csrc/hifigan.hip) at V1 on 1 x 200, 32 x 1000
and 128 x 1000 frames -- the whole call with its multiply-adds and the share of the fp32 MFMA peak (157.3 TFLOP/s) they amount to, and
every launch of it alone (gsttaco_hifigan_debug_stage), summed per stage and kind -- beside the MelGAN generator (Neural_Vocoder),
WaveGlow and the 60 Griffin-Lim iterations (Inv_Spectrogram) of the same batch in the same process.  Every call is timed on its own
between two events: ROUNDS rounds of CALLS calls after a warm-up, the median of all calls and the spread of the rounds' medians
(WaveGlow, seconds a call, and the single launches: one round of three).
python tools/hifigan_time.py [v1|v2|v3] [B x T ...]        (default: v1 1x200 32x1000 128x1000)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from gst_tacotron_amd import capi, hifigan, melgan, synthetic, waveglow, weights
from gst_tacotron_amd.model import GST_Tacotron, _ptr

ROUNDS, CALLS = 3, 5
args = [a.lower() for a in sys.argv[1:]]
which = next((a for a in args if a in ("v1", "v2", "v3")), "v1")
SHAPES = tuple(tuple(int(v) for v in a.split("x")) for a in args if "x" in a) or ((1, 200), (32, 1000), (128, 1000))
Tv, Tref = 128, 64
PEAK = 157.3e12

hp = synthetic.config_hp("cfg2")
hop = hp["Sound"]["Frame_Shift"]
cfg = getattr(hifigan.HiFiGANConfig, which)()
Bmax, Tmax = max(b for b, _ in SHAPES), max(t for _, t in SHAPES)
rng = np.random.default_rng(1)
m = GST_Tacotron(hyper_parameters=hp, max_batch=Bmax, max_tokens=Tv, max_ref_frames=Tref + 1, max_wav_seconds=hop * Tmax / hp["Sound"]["Sample_Rate"] + 1)
m.Restore(weights=weights.synthetic_weights(hp, seed=0))
m.Load_HiFiGAN(hifigan.synthetic_weights(cfg, seed=0), config=cfg, max_frames=Tmax)
m.Load_Neural_Vocoder(melgan.synthetic_weights(melgan.MelGANConfig(), seed=0), max_frames=Tmax)
have_waveglow = True
try:
    m.Load_WaveGlow(waveglow.synthetic_weights(waveglow.WaveGlowConfig(), seed=0), config=waveglow.WaveGlowConfig(), max_frames=Tmax)
except capi.GstTacoError as e:                      # (its workspace beside the other two: the other figures still stand)
    print("WaveGlow not loaded (%s)" % str(e)[:120])
    have_waveglow = False
_, _, stages = m.ctx.hifigan_plan()
mel = m._dev(np.clip(rng.normal(0.0, 1.5, (Bmax, Tmax, 80)), -4, 4).astype(np.float32), torch.float32)
spec = torch.rand((Bmax, Tmax, hp["Sound"]["Spectrogram_Dim"]), device=m.device) * 8 - 4

# multiply-adds per mel frame of each launch, and the group (stage, kind) its time is summed under
ch, macs, groups, rate, up = cfg.channels(), [], [], 1, -1
for s in stages:
    if s["kind"] == "in":
        macs.append(7 * cfg.mel_dim * ch[0]); groups.append("input conv")
    elif s["kind"] == "up":
        up += 1
        rate *= cfg.rates[up]
        macs.append(2 * ch[up] * ch[up + 1] * rate); groups.append("stage %d transposed conv, %d -> %d ch" % (up, ch[up], ch[up + 1]))
    elif s["kind"] == "conv":
        macs.append(s["taps"] * s["channels"] ** 2 * rate); groups.append("stage %d residual convs, %d ch, tile %d, form %d" % (up, s["channels"], s["tile"], s["form"]))
    else:
        macs.append(7 * ch[-1] * rate); groups.append("output conv")
print("HiFi-GAN %s: %d launches, %.1f M multiply-adds a frame (%.2f M a sample), %.1f%% of them in the residual convs; workspace %.1f GB" %
      (which.upper(), len(stages), sum(macs) / 1e6, sum(macs) / hop / 1e6,
       100.0 * sum(v for v, s in zip(macs, stages) if s["kind"] == "conv") / sum(macs),
       4 * 4 * Bmax * Tmax * max(r * 16 * ((c + 15) // 16) for r, c in zip(np.cumprod(cfg.rates), ch[1:])) / 1e9))


def timed(f, rounds=ROUNDS, calls=CALLS, warm=2):
    for i in range(warm):
        f(i)
    torch.cuda.synchronize()
    out = []
    for r in range(rounds):
        ms = []
        for i in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(100 + r * calls + i)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out.append(ms)
    med = [float(np.median(r)) for r in out]
    return float(np.median(np.concatenate(out))), min(med), max(med)


for B, T in SHAPES:
    x = mel[:B, :T].contiguous()
    sp = spec[:B, :T].contiguous()
    frames = m._dev(np.full(B, T, np.int32), torch.int32)
    wav = torch.empty((B, T * hop), dtype=torch.float32, device=m.device)

    def stage(k):
        m.ctx.check(m.ctx.lib.gsttaco_hifigan_debug_stage(m.ctx.handle, k, _ptr(x), None, B, T, _ptr(wav), T * hop, m._stream()))

    res = {"HiFiGAN": timed(lambda i: m.HiFiGAN(x)),
           "Neural_Vocoder (MelGAN)": timed(lambda i: m.Neural_Vocoder(x)),
           "Inv_Spectrogram (60 iterations)": timed(lambda i: m.Inv_Spectrogram(sp, frames=frames, seed=i))}
    if have_waveglow:
        res["WaveGlow"] = timed(lambda i: m.WaveGlow(x, seeds=[i] * B), rounds=1, calls=3, warm=1)
    voc = res["HiFiGAN"][0]
    flop = 2 * sum(macs) * B * T
    print("batch %d x %d frames: %.2f TFLOP a call, %.1f TFLOP/s = %.3f of the fp32 MFMA peak, %.1f k frames/s, %.1f x real time a row at 16 kHz"
          % (B, T, flop / 1e12, flop / voc / 1e9, flop / voc / 1e-3 / PEAK, B * T / voc, T * hop / 16000.0 / (voc * 1e-3)))
    for k, (med, lo, hi) in res.items():
        print("  %-34s median %10.3f ms, round medians %10.3f .. %10.3f, %8.3f of the HiFiGAN" % (k, med, lo, hi, med / voc))
    m.HiFiGAN(x)                                # the workspace now holds this shape's activations
    sums, order = {}, []
    for k, s in enumerate(stages):
        med, _, _ = timed(lambda i: stage(k), rounds=1, calls=3, warm=1)
        if groups[k] not in sums:
            sums[groups[k]] = [0.0, 0.0, 0]
            order.append(groups[k])
        g = sums[groups[k]]
        g[0] += med; g[1] += macs[k]; g[2] += 1
    for name in order:
        ms, mac, n = sums[name]
        print("    %-52s %3d launches %9.3f ms, %7.1f M multiply-adds a frame, %.3f of the peak" %
              (name, n, ms, mac / 1e6, 2 * mac * B * T / (ms * 1e-3) / PEAK))
    print("    sum of the launches %.3f ms" % sum(v[0] for v in sums.values()))
m.synchronize()
