"""What the style map costs beside the embeddings it draws: Style_Affinities (gsttaco_style_affinities, perplexity 5) and 1000 steps of
Style_Map (gsttaco_style_map, the defaults of reference R_Script/TSNE.R) at N = 256, 1024 and 4096 embeddings of D = 256 channels
(csrc/tsne.hip), beside the Inference_GST_Step of the same rows (cfg2, reference mels of 64 frames, in batches of 32) in the same
process, and beside the NumPy restatement of tests/style_map_cases.py on the host for the N it finishes within a minute (10 steps
timed, multiplied out).  The embeddings are three well separated clusters.  Every device call is timed on its own between two events:
ROUNDS rounds of CALLS calls after a warm-up, the median of all calls and the spread of the rounds' medians; the 1000 steps are one
call (2000 launches and the four of the KL divergence).
python tools/style_map_time.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from gst_tacotron_amd import synthetic, weights
from gst_tacotron_amd.model import GST_Tacotron

ROUNDS, CALLS = 3, 5
SIZES, D, BATCH, Tref, STEPS = (256, 1024, 4096), 256, 32, 64, 1000
HOST_BUDGET_S = 60.0

hp = synthetic.config_hp("cfg2")
m = GST_Tacotron(hyper_parameters=hp, max_batch=BATCH, max_tokens=16, max_ref_frames=Tref + 1, max_wav_seconds=0.0)
m.Restore(weights=weights.synthetic_weights(hp, seed=0))
print("embeddings timed: D = %d channels (this configuration's Attention.Size is %d)" % (D, m.dims.gst_att))
rng = np.random.default_rng(1)
mels, ml = synthetic.make_ref_mels(rng, BATCH, Tref)
mels, ml = m._dev(mels, torch.float32), m._dev(ml, torch.int32)


def timed(f, rounds=ROUNDS, calls=CALLS):
    f()
    torch.cuda.synchronize()
    out = []
    for r in range(rounds):
        ms = []
        for i in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out.append(ms)
    med = [float(np.median(r)) for r in out]
    return float(np.median(np.concatenate(out))), min(med), max(med)


import style_map_cases as S
step_ms = timed(lambda: m.Inference_GST_Step(mels, ml), 5, 10)
print("Inference_GST_Step, %d rows x %d frames: median %.3f ms (round medians %.3f .. %.3f)" % ((BATCH, Tref) + step_ms))
for N in SIZES:
    centres = rng.normal(0.0, 4.0, (3, D))
    x = (centres[rng.integers(0, 3, N)] + rng.standard_normal((N, D))).astype(np.float32)
    xd = m._dev(x, torch.float32)
    p, beta, rounds = m.Style_Affinities(xd)
    aff = timed(lambda: m.Style_Affinities(xd))
    run = timed(lambda: m.Style_Map(affinities=p, iters=STEPS))
    res = m.Style_Map(affinities=p, iters=STEPS)
    gst = step_ms[0] * N / BATCH
    print("N = %d: search rounds %d .. %d, KL after %d steps %.4f" % (N, int(rounds.min()), int(rounds.max()), STEPS, float(res["kl"])))
    print("  %-34s median %10.3f ms (round medians %10.3f .. %10.3f), %7.3f of the Inference_GST_Step of %d rows (%.1f ms)" %
          (("Style_Affinities",) + aff + (aff[0] / gst, N, gst)))
    print("  %-34s median %10.3f ms (round medians %10.3f .. %10.3f), %7.3f of it; %.2f us a step" %
          (("Style_Map, %d steps" % STEPS,) + run + (run[0] / gst, 1e3 * run[0] / STEPS)))
    # the host: skipped where 10 steps at about 0.3 us a pair would exceed the budget
    if N * N * 3e-7 * 10 > HOST_BUDGET_S:
        print("  NumPy restatement on the host: not run (beyond %d s)" % HOST_BUDGET_S)
        continue
    t0 = time.perf_counter()
    ref = S.affinities_reference(x, 5.0)
    t_aff = time.perf_counter() - t0
    t0 = time.perf_counter()
    S.descent_reference(ref["p"], S.default_init(N, 0), np.zeros((N, 2)), np.ones((N, 2)), 0, 10)
    t_run = (time.perf_counter() - t0) * STEPS / 10
    same = bool(np.array_equal(ref["beta"], beta.cpu().numpy()))
    print("  NumPy restatement on the host: affinities %.2f s, %d steps %.1f s (10 timed); device beta bitwise the host's: %s" %
          (t_aff, STEPS, t_run, same))
m.synchronize()
