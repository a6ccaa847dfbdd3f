"""What the flow vocoder costs beside the synthesis it voices: gsttaco_waveglow (csrc/waveglow.hip) at the default sizes on 1 x 200,
32 x 1000 and 128 x 1000 frames -- the whole call with its multiply-adds and the share of the fp32 MFMA peak (157.3 TFLOP/s) they
amount to, and, through gsttaco_waveglow_debug_stage, one launch of every distinct form alone (the upsampler, the first flow tail, the
NL layers of the first flow run -- one per dilation -- and one flow tail per channel count) -- beside the MelGAN generator
(Neural_Vocoder) and the Inference_Step (128 tokens, the headline configuration, steps = frames / 2) of the same batch in the same
process.  Every call is timed on its own between two events: ROUNDS rounds of CALLS calls after a warm-up of every form, the median of
all calls and the spread of the rounds' medians.  A batch whose workspace the device cannot hold is halved until it fits, and said so.
python tools/waveglow_time.py [B x T ...]        (default: 1x200 32x1000 128x1000)"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from gst_tacotron_amd import capi, melgan, synthetic, waveglow, weights
from gst_tacotron_amd.model import GST_Tacotron, _ptr

ROUNDS, CALLS = 3, 5
SHAPES = tuple(tuple(int(v) for v in a.lower().split("x")) for a in sys.argv[1:]) or ((1, 200), (32, 1000), (128, 1000))
Tv, Tref = 128, 64
PEAK = 157.3e12

hp = synthetic.config_hp("cfg2")
hop = hp["Sound"]["Frame_Shift"]
cfg = waveglow.WaveGlowConfig()
Bmax, Tmax = max(b for b, _ in SHAPES), max(t for _, t in SHAPES)
rng = np.random.default_rng(1)
wg_weights = waveglow.synthetic_weights(cfg, seed=0)
while True:
    m = GST_Tacotron(hyper_parameters=hp, max_batch=Bmax, max_tokens=Tv, max_ref_frames=Tref + 1, max_wav_seconds=hop * Tmax / hp["Sound"]["Sample_Rate"] + 1)
    m.Restore(weights=weights.synthetic_weights(hp, seed=0))
    try:
        m.Load_WaveGlow(wg_weights, config=cfg, max_frames=Tmax)
        break
    except capi.GstTacoError as e:                  # the capacity formula asks for more than the device has: halve the batch
        print("capacity %d x %d frames: %s -- halving the batch" % (Bmax, Tmax, str(e)[:120]))
        m.ctx.close()
        Bmax //= 2
        if Bmax < 1:
            raise
per_column = 16 * ((cfg.spect_dim + 15) // 16) + 3 * 16 * ((cfg.n_channels + 15) // 16) + 16
print("workspace: %d floats a column, %.1f GB for %d x %d frames" % (per_column, per_column * 4 * Bmax * Tmax * (hop // cfg.n_group) / 1e9, Bmax, Tmax))
m.Load_Neural_Vocoder(melgan.synthetic_weights(melgan.MelGANConfig(), seed=0), max_frames=Tmax)
_, G, stages = m.ctx.waveglow_plan()
tokens, _ = synthetic.make_tokens(rng, Bmax, Tv)
ref, ml = synthetic.make_ref_mels(rng, Bmax, Tref)
tokens, ref, ml = m._dev(tokens, torch.int32), m._dev(ref, torch.float32), m._dev(ml, torch.int32)
mel = m._dev(rng.uniform(-4, 4, (Bmax, Tmax, 80)).astype(np.float32), torch.float32)

# multiply-adds per waveform sample: the WN layers (what the issue's arithmetic counts), and per launch
C, S, NL, F = cfg.n_channels, cfg.spect_dim, cfg.n_layers, cfg.n_flows
layer_macs = [((3 * C + S) * 2 * C + C * (2 * C if i < NL - 1 else C)) / G for i in range(NL)]
macs_sample = cfg.macs_per_sample()
up_macs = (cfg.win // cfg.hop) * cfg.mel_dim * cfg.mel_dim
# one launch of every distinct form: index into the plan's launch order [up, flow, (NL layers, flow) x F]
distinct = [0, 1] + list(range(2, 2 + NL))
seen = set()
for k in range(F):
    idx = 2 + k * (NL + 1) + NL
    if stages[idx]["channels"] not in seen:
        seen.add(stages[idx]["channels"])
        distinct.append(idx)


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
    if B > Bmax:
        print("batch %d x %d frames does not fit: the largest batch that does is %d" % (B, T, Bmax))
        B = Bmax
    x = mel[:B, :T].contiguous()
    wav = torch.empty((B, T * hop), dtype=torch.float32, device=m.device)
    seeds = torch.zeros((B,), dtype=torch.int64, device=m.device)

    def stage(k):
        m.ctx.check(m.ctx.lib.gsttaco_waveglow_debug_stage(m.ctx.handle, k, _ptr(x), None, B, T, ctypes.c_float(0.6), _ptr(seeds), None,
                                                           _ptr(wav), T * hop, m._stream()))

    forms = {"Inference_Step (%d steps)" % (T // 2): lambda i: m.Inference_Step(tokens[:B], None, None, ref[:B], ml[:B], seed=i, steps=T // 2),
             "Neural_Vocoder (MelGAN)": lambda i: m.Neural_Vocoder(x),
             "WaveGlow": lambda i: m.WaveGlow(x, seeds=[i] * B)}
    res = {}
    for k, f in forms.items():
        try:
            res[k] = timed(f)
        except Exception as e:                   # (a batch the decode's capacity does not take: the other figures still stand)
            print("  %s: not run (%s)" % (k, str(e)[:100]))
    voc = res["WaveGlow"][0]
    flop = 2 * macs_sample * B * T * hop
    print("batch %d x %d frames: %.2f M multiply-adds a sample, %.1f TFLOP a call, %.1f TFLOP/s = %.3f of the fp32 MFMA peak, %.1f k frames/s, "
          "%.2f x real time a row at 16 kHz" % (B, T, macs_sample / 1e6, flop / 1e12, flop / voc / 1e9, flop / voc / 1e-3 / PEAK, B * T / voc,
                                              T * hop / 16000.0 / (voc * 1e-3)))
    for k, (med, lo, hi) in res.items():
        print("  %-34s median %10.3f ms of %d x %d calls, round medians %10.3f .. %10.3f, %9.4f of the WaveGlow" %
              (k, med, ROUNDS, CALLS, lo, hi, med / voc))
    m.WaveGlow(x)                               # the workspace now holds this shape's activations
    for k in distinct:
        s = stages[k]
        med, lo, hi = timed(lambda i: stage(k))
        if s["kind"] == "layer":
            i = (k - 2) % (NL + 1)
            mac = layer_macs[i] * B * T * hop
            note = "dilation %3d, %.3f of the peak" % (2 ** i, 2 * mac / (med * 1e-3) / PEAK)
        elif s["kind"] == "up":
            note = "%.3f of the peak" % (2 * up_macs * B * T * hop / (med * 1e-3) / PEAK)
        else:
            note = "VALU"
        print("    launch %3d %-5s %4d ch, tile %3d, form %d: %9.3f ms (%9.3f .. %9.3f)  %s" % (k, s["kind"], s["channels"], s["tile"], s["form"], med, lo, hi, note))
m.synchronize()
