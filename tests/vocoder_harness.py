"""The context wrapper the three vocoders' GPU tests share (tests/test_gpu_melgan.py, test_gpu_hifigan.py, test_gpu_waveglow.py,
test_gpu_hifigan_half.py, test_gpu_vocoder_surface.py; tools/vocoder_bits.py runs the case tables through it too): a context that
holds nothing but one finalized vocoder, called with host arrays, its outputs prefilled with NaN / -1 so that what a call leaves
unwritten shows; and HiFi-GAN's one-launch-alone route (``stage`` / ``buffer``)."""
import ctypes

import numpy as np

from gst_tacotron_amd import capi, synthetic


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def seeds_tensor(vals):
    """uint64 seeds as the int64 device tensor whose bits they are"""
    import torch
    return torch.from_numpy(np.array([int(v) & (2 ** 64 - 1) for v in vals], dtype=np.uint64).view(np.int64)).cuda()


class Vocoder:
    """``prefix`` is "melgan", "hifigan" or "waveglow".  ``raw`` is the C call itself, positional as the C signature is:
    (x, fr, B, T, wav, lens, ld), and for waveglow (x, fr, B, T, sigma, seeds, z, wav, lens, ld); it returns the code."""

    def __init__(self, prefix, cfg, weights, max_batch, max_frames, finalize=True, operands=None):
        self.prefix, self.cfg, self.max_batch, self.max_frames = prefix, cfg, max_batch, max_frames
        self.ctx = capi.Context(synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4)
        getattr(self.ctx, prefix + "_configure")(cfg, max_batch, max_frames)
        if operands is not None:            # hifigan: the operand form, chosen between configure and finalize
            self.ctx.hifigan_set_operands(operands)
        getattr(self.ctx, prefix + "_load_weights")(weights)
        if finalize:
            getattr(self.ctx, prefix + "_finalize")()

    def raw(self, x, fr, B, T, *rest, stream=None):
        import torch
        s = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        want = 6 if self.prefix == "waveglow" else 3
        if len(rest) != want:
            raise TypeError("{}: raw takes (x, fr, B, T, {}wav, lens, ld), got {} arguments behind T".format(
                self.prefix, "sigma, seeds, z, " if want == 6 else "", len(rest)))
        if self.prefix == "waveglow":
            sigma, seeds, z, wav, lens, ld = rest
            return self.ctx.lib.gsttaco_waveglow(self.ctx.handle, _p(x), _p(fr), B, T, ctypes.c_float(sigma), _p(seeds), _p(z), _p(wav), _p(lens), ld, s)
        wav, lens, ld = rest
        return getattr(self.ctx.lib, "gsttaco_" + self.prefix)(self.ctx.handle, _p(x), _p(fr), B, T, _p(wav), _p(lens), ld, s)

    def stage(self, i, x, fr, B, T, wav, ld):
        """hifigan: launch i of the plan alone (gsttaco_hifigan_debug_stage) on the workspace as it stands"""
        import torch
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.ctx.check(self.ctx.lib.gsttaco_hifigan_debug_stage(self.ctx.handle, i, _p(x), _p(fr), B, T, _p(wav), ld, s))

    def buffer(self, k, tensor, write):
        """hifigan: the float32 device ``tensor`` into (``write``) or out of workspace buffer k (gsttaco_hifigan_debug_buffer)"""
        import torch
        self.ctx.hifigan_debug_buffer(k, tensor, write, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def noise(self, seeds, T):
        """waveglow: z [len(seeds), T * hop] as gsttaco_waveglow_noise draws it"""
        import torch
        sd = seeds_tensor(seeds)
        z = torch.full((len(seeds), T * self.cfg.hop), float("nan"), dtype=torch.float32, device="cuda")
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.ctx.check(self.ctx.lib.gsttaco_waveglow_noise(self.ctx.handle, _p(sd), len(seeds), T, _p(z), s))
        torch.cuda.synchronize()
        return z.cpu().numpy()

    def __call__(self, mel, frames=None, z=None, seeds=None, sigma=0.6, ld=None):
        """(wav [B, ld], lengths [B]) as host arrays.  z / seeds / sigma are waveglow's."""
        import torch
        x = torch.as_tensor(np.ascontiguousarray(mel, dtype=np.float32)).cuda()
        B, T = x.shape[:2]
        fr = None if frames is None else torch.as_tensor(np.asarray(frames, dtype=np.int32)).cuda()
        ld = T * self.cfg.hop if ld is None else ld
        wav = torch.full((B, ld), float("nan"), dtype=torch.float32, device="cuda")
        lens = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        if self.prefix == "waveglow":
            zd = None if z is None else torch.as_tensor(np.ascontiguousarray(z, dtype=np.float32)).cuda()
            sd = None if seeds is None else seeds_tensor(seeds)
            rc = self.raw(x, fr, B, T, sigma, sd, zd, wav, lens, ld)
        else:
            rc = self.raw(x, fr, B, T, wav, lens, ld)
        self.ctx.check(rc)
        torch.cuda.synchronize()
        return wav.cpu().numpy(), lens.cpu().numpy()

    def close(self):
        self.ctx.close()
