"""What the validation losses cost at 32 utterances x 1000 frames (Mel_Dim 80, Spectrogram_Dim 513): gsttaco_losses with and without the
spectrogram pair, beside a device-to-device copy of the spectrogram tensor as the yardstick, and gsttaco_feature_frontend beside
gsttaco_mel_frontend on 32 wavs of 16 s (1000 frames each).  CALLS launches between two events, REPEATS blocks.
python tools/eval_time.py"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gst_tacotron_amd import hparams
from gst_tacotron_amd.model import GST_Tacotron

CALLS, REPEATS = 20, 5
B, T = 32, 1000

hp = hparams.load_hp()
hp["Step_Reduction"], hp["Max_Step"] = 1, T
m = GST_Tacotron(hyper_parameters=hp, max_batch=B, max_tokens=8, max_ref_frames=4, max_wav_seconds=17.0)     # (no weights: none are needed)
d = m.dims
rng = np.random.default_rng(3)
dev = lambda *shape: torch.from_numpy(rng.normal(0.0, 1.5, shape).astype(np.float32)).cuda()
pre, mel, spec, stop = dev(B, T, d.mel), dev(B, T, d.mel), dev(B, T, d.spec), dev(B, T)
teacher, target = dev(B, T + 1, d.mel), dev(B, T + 1, d.spec)
lengths = torch.from_numpy(rng.integers(T // 2, T + 1, B).astype(np.int32)).cuda()
copy = torch.empty_like(spec)
read_mb = (3 * B * T * d.mel + 2 * B * T * d.spec) * 4 / 1e6

ld = d.frame_shift * T
wav = torch.from_numpy((0.1 * rng.standard_normal((B, ld))).astype(np.float32)).cuda()
wav_len = torch.full((B,), ld, dtype=torch.int32).cuda()
cap = 2 + ld // d.frame_shift
fmel = torch.empty(B, cap, d.mel).cuda()
fspec = torch.empty(B, cap, d.spec).cuda()
flen = torch.empty(B, dtype=torch.int32).cuda()
p = lambda t: ctypes.c_void_p(t.data_ptr())
lib, h, top_db = m.ctx.lib, m.ctx.handle, ctypes.c_float(15.0)

forms = {"losses, mel + spectrogram (%.0f MB read)" % read_mb: lambda: m.Loss_Terms(pre, mel, stop, teacher, lengths, spec, target, lengths),
         "losses, mel only": lambda: m.Loss_Terms(pre, mel, stop, teacher, lengths),
         "copy of the spectrograms (d2d, %.0f MB)" % (B * T * d.spec * 4 / 1e6): lambda: copy.copy_(spec),
         "mel front end (3 kernels)": lambda: m.ctx.check(lib.gsttaco_mel_frontend(h, p(wav), p(wav_len), B, ld, top_db, p(fmel), p(flen), cap, m._stream())),
         "feature front end: mel + spectrogram": lambda: m.ctx.check(lib.gsttaco_feature_frontend(h, p(wav), p(wav_len), B, ld, top_db, p(fmel), p(fspec), p(flen),
                                                                                                  cap, m._stream()))}
for f in forms.values():
    f()
torch.cuda.synchronize()
print("frames per wav:", flen.cpu().tolist()[:4], "...; loss sums of row 0:", m.Loss_Terms(pre, mel, stop, teacher, lengths, spec, target, lengths)[0].tolist())
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
    print("%-48s median %8.1f us per call, blocks min %8.1f max %8.1f" % (k, float(np.median(us)), min(us), max(us)))
