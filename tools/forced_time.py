"""What teacher forcing costs: Inference_Step(teacher_mels=) at 32 utterances x 128 tokens x 500 steps (1000 frames) against the free
run of the same shape on the launch path (GSTTACO_PERSIST_DECODE=0: the forced call never takes the persistent launch), on one
model of one build.  The forced call adds two launches in front of the loop (the teacher gather, the Z0 GEMM) and takes the 80-wide
prenet-0 product out of every step.  Blocks of CALLS calls between two events, the two forms alternating, REPEATS blocks each: the
spread of the free run's own blocks is printed beside the difference.    python tools/forced_time.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["GSTTACO_PERSIST_DECODE"] = "0"
import numpy as np, torch
from gst_tacotron_amd import synthetic, weights
from gst_tacotron_amd.model import GST_Tacotron

CALLS, REPEATS = 10, 5
B, Tv, Tref, STEPS = 32, 128, 64, 500

hp = synthetic.config_hp("cfg2")
r, mel = hp["Step_Reduction"], hp["Sound"]["Mel_Dim"]
rng = np.random.default_rng(1)
tokens, _ = synthetic.make_tokens(rng, B, Tv)
mels, ml = synthetic.make_ref_mels(rng, B, Tref)
teacher = np.clip(rng.normal(0.0, 1.5, (B, 1 + STEPS * r, mel)), -4.0, 4.0).astype(np.float32)
m = GST_Tacotron(hyper_parameters=hp, max_batch=B, max_tokens=Tv, max_ref_frames=Tref + 1)
m.Restore(weights=weights.synthetic_weights(hp, seed=0))
tokens, mels, ml, teacher = m._dev(tokens, torch.int32), m._dev(mels, torch.float32), m._dev(ml, torch.int32), m._dev(teacher, torch.float32)
forms = {"free run (launch path)": lambda i: m.Inference_Step(tokens, None, None, mels, ml, seed=i, steps=STEPS),
         "teacher-forced": lambda i: m.Inference_Step(tokens, None, None, mels, ml, seed=i, teacher_mels=teacher)}
for f in forms.values():
    for i in range(3):
        f(i)
m.synchronize()
assert m.decode_counters()[0] == 0
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
    print("%-24s median %8.3f ms per Inference_Step, blocks min %8.3f max %8.3f" % (k, float(np.median(v)), min(v), max(v)))
free, forced = ms["free run (launch path)"], ms["teacher-forced"]
print("teacher-forced - free run: %+.3f ms (medians); spread of the free run's blocks %.3f ms" %
      (float(np.median(forced) - np.median(free)), max(free) - min(free)))
