"""What the HiFi-GAN vocoder costs, in its three operand forms and beside the other ways to a waveform: gsttaco_hifigan
(csrc/hifigan.hip) at V1 on 1 x 200, 32 x 1000 and 128 x 1000 frames.
  - The three forms side by side in one process: a context each for float32, bfloat16 and float16 operands
    (gsttaco_hifigan_set_operands), called in turn -- ROUNDS rounds of CALLS calls a form, the forms alternating round by round, every
    call between two events after a warm-up; the median of all calls and the spread of the rounds' medians.  The float32 row is the
    baseline of the same run.
  - Every launch of --precision's form alone (gsttaco_hifigan_debug_stage), summed per stage and kind, with the share of the MFMA peak
    of that form (157.3 TFLOP/s fp32, 2516.6 TFLOP/s 16-bit) and the share of HBM_RATE that the launch's minimal traffic (its input
    read once, its residual and sum where it has them, its output written once, fp32) amounts to.
  - Beside them the MelGAN generator (Neural_Vocoder), WaveGlow and the 60 Griffin-Lim iterations (Inv_Spectrogram) of the same batch
    (skipped with --only-hifigan).
python tools/hifigan_time.py [v1|v2|v3] [B x T ...] [--precision float32|bfloat16|float16] [--only-hifigan]
                                                                                  (default: v1 1x200 32x1000 128x1000, float32)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from gst_tacotron_amd import capi, hifigan, melgan, synthetic, waveglow, weights
from gst_tacotron_amd.model import GST_Tacotron, _ptr

ROUNDS, CALLS = 3, 5
argv = sys.argv[1:]
precision = "float32"
if "--precision" in argv:
    precision = hifigan.check_precision(argv[argv.index("--precision") + 1])
    del argv[argv.index("--precision"):argv.index("--precision") + 2]
only = "--only-hifigan" in argv
args = [a.lower() for a in argv if not a.startswith("--")]
which = next((a for a in args if a in ("v1", "v2", "v3")), "v1")
SHAPES = tuple(tuple(int(v) for v in a.split("x")) for a in args if "x" in a) or ((1, 200), (32, 1000), (128, 1000))
Tv, Tref = 128, 64
PEAK = {"float32": 157.3e12, "bfloat16": 2516.6e12, "float16": 2516.6e12}
HBM_RATE = 6.3e12               # bytes/s a streaming copy reaches on this chip (8.0e12 on paper): the shares below are of this figure

hp = synthetic.config_hp("cfg2")
hop = hp["Sound"]["Frame_Shift"]
cfg = getattr(hifigan.HiFiGANConfig, which)()
Bmax, Tmax = max(b for b, _ in SHAPES), max(t for _, t in SHAPES)
rng = np.random.default_rng(1)
vw = hifigan.synthetic_weights(cfg, seed=0)
models = {}
for p in hifigan.PRECISIONS:        # one context a form: the form is fixed at finalize
    m = GST_Tacotron(hyper_parameters=hp, max_batch=Bmax, max_tokens=Tv, max_ref_frames=Tref + 1,
                     max_wav_seconds=(hop * Tmax / hp["Sound"]["Sample_Rate"] + 1) if p == "float32" and not only else 0.0)
    if p == "float32" and not only:
        m.Restore(weights=weights.synthetic_weights(hp, seed=0))
    m.Load_HiFiGAN(vw, config=cfg, max_frames=Tmax, precision=p)
    models[p] = m
m = models["float32"]
have_waveglow = not only
if not only:
    m.Load_Neural_Vocoder(melgan.synthetic_weights(melgan.MelGANConfig(), seed=0), max_frames=Tmax)
    try:
        m.Load_WaveGlow(waveglow.synthetic_weights(waveglow.WaveGlowConfig(), seed=0), config=waveglow.WaveGlowConfig(), max_frames=Tmax)
    except capi.GstTacoError as e:                      # (its workspace beside the others: the other figures still stand)
        print("WaveGlow not loaded (%s)" % str(e)[:120])
        have_waveglow = False
_, _, stages = models[precision].ctx.hifigan_plan()
mel = m._dev(np.clip(rng.normal(0.0, 1.5, (Bmax, Tmax, 80)), -4, 4).astype(np.float32), torch.float32)
spec = torch.rand((Bmax, Tmax, hp["Sound"]["Spectrogram_Dim"]), device=m.device) * 8 - 4

# multiply-adds and minimal fp32 bytes per mel frame of each launch, and the group (stage, kind) its time is summed under
ch, macs, byts, groups, rate, up = cfg.channels(), [], [], [], 1, -1
p16 = lambda c: 16 * ((c + 15) // 16)
for s in stages:
    if s["kind"] == "in":
        macs.append(7 * cfg.mel_dim * ch[0]); groups.append("input conv"); byts.append(4 * (cfg.mel_dim + p16(ch[0])))
    elif s["kind"] == "up":
        up += 1
        byts.append(4 * (rate * p16(ch[up]) + rate * cfg.rates[up] * p16(ch[up + 1])))
        rate *= cfg.rates[up]
        macs.append(2 * ch[up] * ch[up + 1] * rate); groups.append("stage %d transposed conv, %d -> %d ch" % (up, ch[up], ch[up + 1]))
    elif s["kind"] == "conv":
        macs.append(s["taps"] * s["channels"] ** 2 * rate); groups.append("stage %d residual convs, %d ch, tile %d, form %d" % (up, s["channels"], s["tile"], s["form"]))
        byts.append(4 * rate * p16(s["channels"]) * 3)          # input, residual or sum, output: three transfers at the least
    else:
        macs.append(7 * ch[-1] * rate); groups.append("output conv"); byts.append(4 * rate * (p16(ch[-1]) + 1))
print("HiFi-GAN %s: %d launches, %.1f M multiply-adds a frame (%.2f M a sample), %.1f%% of them in the residual convs; workspace %.1f GB a form" %
      (which.upper(), len(stages), sum(macs) / 1e6, sum(macs) / hop / 1e6,
       100.0 * sum(v for v, s in zip(macs, stages) if s["kind"] == "conv") / sum(macs),
       4 * 4 * Bmax * Tmax * max(r * 16 * ((c + 15) // 16) for r, c in zip(np.cumprod(cfg.rates), ch[1:])) / 1e9))


def timed(f, rounds=ROUNDS, calls=CALLS, warm=2):
    return timed_many({"": f}, rounds, calls, warm)[""]


def timed_many(fs, rounds=ROUNDS, calls=CALLS, warm=2):
    """{name: f} -> {name: (median, least and largest round median)}; the names alternate round by round"""
    for f in fs.values():
        for i in range(warm):
            f(i)
    torch.cuda.synchronize()
    out = {k: [] for k in fs}
    for r in range(rounds):
        for k, f in fs.items():
            ms = []
            for i in range(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f(100 + r * calls + i)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            out[k].append(ms)
    res = {}
    for k, v in out.items():
        med = [float(np.median(r)) for r in v]
        res[k] = (float(np.median(np.concatenate(v))), min(med), max(med))
    return res


for B, T in SHAPES:
    x = mel[:B, :T].contiguous()
    sp = spec[:B, :T].contiguous()
    frames = m._dev(np.full(B, T, np.int32), torch.int32)
    wav = torch.empty((B, T * hop), dtype=torch.float32, device=m.device)
    mp = models[precision]

    def stage(k):
        mp.ctx.check(mp.ctx.lib.gsttaco_hifigan_debug_stage(mp.ctx.handle, k, _ptr(x), None, B, T, _ptr(wav), T * hop, mp._stream()))

    forms = timed_many({p: (lambda i, mm=models[p]: mm.HiFiGAN(x)) for p in hifigan.PRECISIONS})
    res = {"HiFiGAN " + p: forms[p] for p in hifigan.PRECISIONS}
    if not only:
        res["Neural_Vocoder (MelGAN)"] = timed(lambda i: m.Neural_Vocoder(x))
        res["Inv_Spectrogram (60 iterations)"] = timed(lambda i: m.Inv_Spectrogram(sp, frames=frames, seed=i))
    if have_waveglow:
        res["WaveGlow"] = timed(lambda i: m.WaveGlow(x, seeds=[i] * B), rounds=1, calls=3, warm=1)
    base = forms["float32"][0]
    flop = 2 * sum(macs) * B * T
    print("batch %d x %d frames: %.2f TFLOP a call, %.2f GB of minimal fp32 activation traffic" % (B, T, flop / 1e12, sum(byts) * B * T / 1e9))
    for p in hifigan.PRECISIONS:
        voc = forms[p][0]
        print("  %-9s %.1f TFLOP/s = %.3f of its MFMA peak, %.2f TB/s = %.3f of %.1f TB/s, %.1f k frames/s, %.1f x real time a row at 16 kHz, %.2f x the float32 form"
              % (p, flop / voc / 1e9, flop / voc / 1e-3 / PEAK[p], sum(byts) * B * T / voc / 1e9, sum(byts) * B * T / (voc * 1e-3) / HBM_RATE,
                 HBM_RATE / 1e12, B * T / voc, T * hop / 16000.0 / (voc * 1e-3), base / voc))
    for k, (med, lo, hi) in res.items():
        print("  %-34s median %10.3f ms, round medians %10.3f .. %10.3f, %8.3f of the float32 HiFiGAN" % (k, med, lo, hi, med / base))
    mp.HiFiGAN(x)                               # the workspace now holds this shape's activations
    sums, order = {}, []
    for k, s in enumerate(stages):
        med, _, _ = timed(lambda i: stage(k), rounds=1, calls=3, warm=1)
        if groups[k] not in sums:
            sums[groups[k]] = [0.0, 0.0, 0, 0.0]
            order.append(groups[k])
        g = sums[groups[k]]
        g[0] += med; g[1] += macs[k]; g[2] += 1; g[3] += byts[k]
    print("    every launch alone, %s operands:" % precision)
    for name in order:
        ms, mac, n, by = sums[name]
        print("    %-52s %3d launches %9.3f ms, %7.1f M multiply-adds a frame, %.3f of the peak, %.3f of the HBM rate" %
              (name, n, ms, mac / 1e6, 2 * mac * B * T / (ms * 1e-3) / PEAK[precision], by * B * T / (ms * 1e-3) / HBM_RATE))
    print("    sum of the launches %.3f ms" % sum(v[0] for v in sums.values()))
for mm in models.values():
    mm.synchronize()
