"""What the synthesis report costs: gsttaco_utterance_report on stop [32, 500] and align [32, 500, 128] (8.2 MB) -- rows that never stop
(all 500 steps read) and rows that stop at step 250 (half of them read) -- beside a device-to-device copy of the same alignment tensor,
i.e. the same bytes read once, as the yardstick.  CALLS launches between two events, REPEATS blocks.    python tools/report_time.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gst_tacotron_amd import synthetic
from gst_tacotron_amd.model import GST_Tacotron

CALLS, REPEATS = 50, 5
B, S, Tv = 32, 500, 128

m = GST_Tacotron(hyper_parameters=synthetic.config_hp("cfg2"), max_batch=B, max_tokens=Tv)       # (no weights: none are needed)
rng = np.random.default_rng(2)
align = torch.from_numpy(rng.random((B, S, Tv)).astype(np.float32)).cuda()
never = torch.ones(B, S).cuda()
half = never.clone()
half[:, 250] = -1.0
mel = torch.zeros(B, S * m.dims.r, m.dims.mel).cuda()
copy = torch.empty_like(align)
forms = {"report, no stop (500 steps read)": lambda: m.Utterance_Report(never, align),
         "report, stop at step 250": lambda: m.Utterance_Report(half, align),
         "report, no stop, with mels": lambda: m.Utterance_Report(never, align, None, mel),
         "copy of the alignments (d2d)": lambda: copy.copy_(align)}
for f in forms.values():
    f()
torch.cuda.synchronize()
rep, foc = m.Utterance_Report(half, align)
print("stop at 250:", dict(zip(("stop_step", "frames"), rep[0, :2].tolist())), "focus", float(foc[0]))
for k, f in forms.items():
    us = []
    for rep in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(CALLS):
            f()
        e1.record()
        e1.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1) / CALLS)
    print("%-36s median %8.1f us per call, blocks min %8.1f max %8.1f" % (k, float(np.median(us)), min(us), max(us)))
