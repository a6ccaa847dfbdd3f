"""What per-utterance seeds cost: Inference_Step(seeds=) at 32 utterances x 128 tokens x 500 steps (1000 frames) against Inference_Step(seed=)
of the same shape, on one model of one build.  The seeded call stages its generated randomness (gsttaco_fill_randomness: 500 x 2 x 32 x 256
keep decisions + 500 x 32 x 128 noise samples, ~41 MB) and decodes with INJECTED masks, so its front launch reads the masks instead of
hashing the decisions and loses the row skipping of the hashed lean front.  Blocks of CALLS calls between two events, the two forms
alternating, REPEATS blocks each: the spread of the single-seed blocks is printed beside the difference.    python tools/seeds_time.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gst_tacotron_amd import synthetic, weights
from gst_tacotron_amd.model import GST_Tacotron

CALLS, REPEATS = 10, 5
B, Tv, Tref, STEPS = 32, 128, 64, 500

hp = synthetic.config_hp("cfg2")
rng = np.random.default_rng(1)
tokens, _ = synthetic.make_tokens(rng, B, Tv)
mels, ml = synthetic.make_ref_mels(rng, B, Tref)
m = GST_Tacotron(hyper_parameters=hp, max_batch=B, max_tokens=Tv, max_ref_frames=Tref + 1)
m.Restore(weights=weights.synthetic_weights(hp, seed=0))
tokens, mels, ml = m._dev(tokens, torch.int32), m._dev(mels, torch.float32), m._dev(ml, torch.int32)
forms = {"seed= (one per call)": lambda i: m.Inference_Step(tokens, None, None, mels, ml, seed=i, steps=STEPS),
         "seeds= (one per utterance)": lambda i: m.Inference_Step(tokens, None, None, mels, ml, seeds=[B * i + b for b in range(B)], steps=STEPS)}
for f in forms.values():
    for i in range(3):
        f(i)
m.synchronize()
print("persistent decode launches after the warm-up: %d, still allowed: %d" % m.decode_counters())
ms = {k: [] for k in forms}
for rep in range(REPEATS):
    for k, f in forms.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(CALLS):
            f(100 * rep + i)
        e1.record()
        e1.synchronize()
        ms[k].append(e0.elapsed_time(e1) / CALLS)
m.synchronize()
for k, v in ms.items():
    print("%-28s median %8.3f ms per Inference_Step, blocks min %8.3f max %8.3f" % (k, float(np.median(v)), min(v), max(v)))
one, per = ms["seed= (one per call)"], ms["seeds= (one per utterance)"]
print("seeds= - seed=: %+.3f ms (medians, %+.1f %%); spread of the single-seed blocks %.3f ms" %
      (float(np.median(per) - np.median(one)), 100.0 * float(np.median(per) / np.median(one) - 1.0), max(one) - min(one)))
# the fill alone
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
m.Fill_Randomness(list(range(B)), STEPS, Tv)
e0.record()
for i in range(20):
    m.Fill_Randomness(list(range(B)), STEPS, Tv)
e1.record()
e1.synchronize()
print("Fill_Randomness alone (host staging of the seeds included): %.3f ms per call" % (e0.elapsed_time(e1) / 20))
