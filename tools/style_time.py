"""What skipping the GST branch is worth: whole Inference_Step at 32 and at 128 utterances x 128 tokens x 1000 frames with a 64-frame
reference, against the same call with the style given (Inference_Step(style_embeddings=Inference_GST_Step(mels))), on one model of
one build.  Blocks of 20 calls between two events, the two forms alternating, REPEATS blocks each: the spread of the reference-audio
call's own blocks is printed beside the difference.    python tools/style_time.py"""
import gc, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gst_tacotron_amd import synthetic, weights
from gst_tacotron_amd.model import GST_Tacotron

CALLS, REPEATS = 20, 5


def run(B, Tv=128, Tref=64):
    hp = synthetic.config_hp("cfg2")
    rng = np.random.default_rng(1)
    tokens, _ = synthetic.make_tokens(rng, B, Tv)
    mels, ml = synthetic.make_ref_mels(rng, B, Tref)
    m = GST_Tacotron(hyper_parameters=hp, max_batch=B, max_tokens=Tv, max_ref_frames=Tref + 1)
    m.Restore(weights=weights.synthetic_weights(hp, seed=0))
    tokens, mels, ml = m._dev(tokens, torch.int32), m._dev(mels, torch.float32), m._dev(ml, torch.int32)
    style = m.Inference_GST_Step(mels, ml)
    forms = {"reference audio": lambda i: m.Inference_Step(tokens, None, None, mels, ml, seed=i),
             "style given": lambda i: m.Inference_Step(tokens, None, None, seed=i, style_embeddings=style)}
    a = forms["reference audio"](7)
    b = forms["style given"](7)
    m.synchronize()
    same = all(torch.equal(x, y) for x, y in zip((a[0], a[1], a[3]), (b[0], b[1], b[3])))
    for f in forms.values():
        for i in range(3):
            f(i)
    m.synchronize()
    ms = {k: [] for k in forms}
    for r in range(REPEATS):
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(CALLS):
                f(100 * r + i)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / CALLS)
    m.synchronize()
    for k, v in ms.items():
        print("B %3d  %-16s median %7.3f ms per Inference_Step, blocks min %7.3f max %7.3f" % (B, k, float(np.median(v)), min(v), max(v)))
    ref, sty = ms["reference audio"], ms["style given"]
    print("B %3d  style given - reference audio: %+.3f ms (medians); spread of the reference-audio blocks %.3f ms; outputs bitwise equal: %s; "
          "persistent decode launches %d" % (B, float(np.median(sty) - np.median(ref)), max(ref) - min(ref), same, m.decode_counters()[0]))
    del m
    gc.collect()        # (the persistent launch is taken only while the process has ONE live context: no lingering one)


for B in (32, 128):
    run(B)
