"""``GST_Tacotron`` -- host-side mirror of the reference class of the same name
(reference Model.py:37-459), inference methods only:

    GST_Tacotron(is_Training=False).Restore(path)
    .Inference_Step(tokens, token_lengths, initial_mels, mels_for_gst, mel_lengths_for_gst)
    .Inference_GST_Step(mels_for_gst, mel_lengths_for_gst)
    .Inference(sentence_List, mel_List_for_GST)
    .Style_Compose(token_weights, query)                 (extension: a style from token weights)
    .Inference_GTA(sentence_List, mel_or_wav_List)       (extension: teacher-forced decoding -- GTA mels, forced durations)
    .Evaluate(sentence_List, mel_or_wav_List)            (extension: Train_Step's loss terms of a teacher-forced pass)
    .Evaluate_Free(sentence_List, mel_or_wav_List)       (extension: MCD along a DTW path of a free run against its target)

Same names, argument order/meaning and error behaviour; the Keras functional model
behind them (Model.py:145-156) is replaced by the HIP kernels behind include/gsttaco.h.
PyTorch is used for device memory and streams only.  Differences, all additive:
  * the config is passed explicitly instead of being read from the CWD at import time;
  * randomness the reference draws unseeded (prenet dropout that is live at inference,
    Taco2.py:283; SMA sigmoid noise, Steps.py:220-221) can be injected (``prenet_masks``,
    ``attn_noise``) for parity runs, otherwise it is generated on the GPU from ``seed``;
  * ``token_lengths`` / ``initial_mels`` are accepted and ignored exactly like the
    reference ignores them at inference (Model.py:249-253, Taco2.py:161);
  * the CBHG vocoder output (3rd element of the returned tuple, Vocoder_Taco1) is computed when
    ``with_vocoder=True`` (gsttaco_vocoder); by default it is None, because the north-star metric
    (mel frames) excludes it;
  * style control: ``Inference_GST_Step(return_attention=True)`` also returns the token weights and the query the
    reference computes and drops (GST.py:105), ``Style_Compose`` builds an embedding from given token weights, and
    ``Inference_Step`` / ``Inference`` take ``style_embeddings`` (and ``Inference`` ``style_token_weights``) in place
    of reference audio;
  * teacher forcing: ``Inference_Step`` / ``decode`` take ``teacher_mels`` -- the decoder then consumes the ground-truth frames like
    the reference's training=True loop branch (Taco2.py:161,185), with every layer still in inference mode --, ``Forced_Durations``
    counts frames per token of an alignment and ``Inference_GTA`` wraps both for ground-truth-aligned mels;
  * per-utterance seeds and a synthesis report: ``seeds=`` ([batch], one per utterance) in place of ``seed`` makes an utterance's
    dropout and noise depend on its own seed alone -- not on its row or the batch --, ``Utterance_Report`` says on the device where each
    utterance stopped and how its attention moved, and ``Inference_Checked`` runs a batch, reads the report and redoes only the
    rejected rows under new seeds;
  * validation losses: ``Evaluate`` runs one teacher-forced pass and returns the four loss terms of the reference's ``Train_Step``
    (Model.py:210-241), per utterance and per batch (``Loss_Terms`` on the device, ``gst_tacotron_amd.evaluate`` on the host);
    ``Feature_Generate`` is ``Mel_Generate`` with the linear spectrogram target from the same STFT;
  * a free-run metric: ``Mel_DTW`` aligns two mel sequences of different lengths on the device (mel-cepstral distortion along a
    dynamic-time-warping path) and ``Evaluate_Free`` reports it for a free-running ``Inference_Step`` against its target;
  * resampling on the device: reference audio that is not at Sound.Sample_Rate -- a wav path at any rate or a ``(samples, rate)``
    pair -- is brought there by ``Resample`` (gsttaco_resample: librosa.core.load's 'kaiser_best') inside ``Mel_Generate`` /
    ``Feature_Generate`` and so behind every method that takes wavs; ``GST_Tacotron(resample="host")`` keeps the NumPy path.
  * prosody metrics: ``Pitch`` / ``Pitch_Signals`` track F0 by YIN on the mel front end's frame grid (gsttaco_pitch), ``Pitch_Errors``
    counts gross pitch, voicing decision and F0 frame errors of two tracks along a DTW path (gsttaco_pitch_errors), and
    ``Evaluate_Free(..., pitch=True)`` reports them beside the MCD -- on the Griffin-Lim waveform of the vocoder's spectrogram.
"""
import ctypes
import os
from datetime import datetime

import numpy as np
import torch

from . import capi, checked, evaluate, weights as weights_mod
from .checked import REPORT_FIELDS  # noqa: F401  -- the columns of Utterance_Report's first result
from .evaluate import FREE_FIELDS, LOSS_FIELDS  # noqa: F401  -- the columns of Evaluate_Free's per_utterance and of Loss_Terms' result
from .feeder import Feeder
from .hparams import Dims, load_hp, load_token_dict


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def style_map_init(n, seed=0):
    """Where ``Style_Map`` starts without an ``init``: N x 2 normal draws of the host's generator, scaled by 1e-4 (bhtsne's scale)."""
    return np.random.default_rng(seed).standard_normal((n, 2)) * 1e-4


class GST_Tacotron:
    def __init__(self, is_Training=False, hyper_parameters=None, device=None,
                 max_batch=32, max_tokens=256, max_ref_frames=1025, max_wav_seconds=20.0, resample="device"):
        if is_Training:
            raise NotImplementedError("only the inference hot path is implemented (training is out of scope)")
        if resample not in ("device", "host"):
            raise ValueError("resample must be 'device' (gsttaco_resample) or 'host' (audio.resample_kaiser_best)")
        self.resample = resample            # where reference audio at another rate is brought to Sound.Sample_Rate (_stage_wavs)
        self.hp_Dict = load_hp(hyper_parameters)
        self.token_Index_Dict = load_token_dict(self.hp_Dict)
        self.dims = Dims(self.hp_Dict, vocab=len(self.token_Index_Dict))
        self.feeder = Feeder(self.hp_Dict, self.token_Index_Dict, mel_frontend=self.Mel_Generate)
        if device is None:
            dev = self.hp_Dict.get("Device", "0")
            device = int(dev) if str(dev).lstrip("-").isdigit() and int(dev) >= 0 else 0
        self.device_index = int(device)
        self.ctx = capi.Context(self.hp_Dict, vocab=len(self.token_Index_Dict), device=self.device_index,
                                max_batch=max_batch, max_tokens=max_tokens, max_ref_frames=max_ref_frames,
                                max_wav_seconds=max_wav_seconds if self.dims.audio else 0.0)
        self._ready = False
        self._melgan = None                 # the loaded neural vocoder's MelGANConfig (Load_Neural_Vocoder)
        self._waveglow = None               # the loaded flow vocoder's WaveGlowConfig (Load_WaveGlow)
        self._hifigan = None                # the loaded HiFi-GAN's HiFiGANConfig (Load_HiFiGAN)
        self._hifigan_precision = None      # and the operand type it was loaded with
        self.seed = 0

    # ------------------------------------------------------------------ weights
    def Restore(self, checkpoint_File_Path=None, weights=None):
        """reference Model.py:267-276.  Loads (a) a flat ``.npz`` weight file (names/shapes:
        gst_tacotron_amd.weights.manifest), (b) a reference ``tf.train.Checkpoint`` prefix (``<prefix>.index`` +
        ``.data-*``, read without TensorFlow by gst_tacotron_amd.tf_checkpoint -- SURVEY N3), (c) with no argument the
        latest checkpoint under ``Checkpoint_Path`` like the reference, or (d) an in-memory dict; prints and returns
        like the reference when nothing is found."""
        from . import tf_checkpoint
        if weights is None:
            if checkpoint_File_Path is None:
                checkpoint_File_Path = tf_checkpoint.latest_checkpoint(self.hp_Dict.get("Checkpoint_Path", "."))   # :268-270
            if checkpoint_File_Path is not None and os.path.exists(str(checkpoint_File_Path) + ".index"):
                # verify=True: every tensor's crc32c is checked (native gsttaco_crc32c), so a truncated or corrupted
                # .data shard fails here instead of loading silently
                weights = tf_checkpoint.load_reference_checkpoint(checkpoint_File_Path, self.hp_Dict,
                                                                  vocab=len(self.token_Index_Dict), verify=True)
            elif checkpoint_File_Path is not None and os.path.exists(checkpoint_File_Path):
                weights = weights_mod.load_npz(checkpoint_File_Path)
            else:
                print("There is no checkpoint.")
                return self
        weights_mod.check_weights(self.hp_Dict, weights, vocab=len(self.token_Index_Dict))
        if not torch.cuda.is_available():
            raise capi.GstTacoError(-2, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)")
        self.ctx.load_weights(weights)
        self.ctx.finalize()
        self._ready = True
        if checkpoint_File_Path is not None:
            print("Checkpoint '{}' is loaded.".format(checkpoint_File_Path))       # reference Model.py:276, after the load
        return self

    # ------------------------------------------------------------------ helpers
    @property
    def device(self):
        return torch.device("cuda", self.device_index)

    def _dev(self, a, dtype):
        if a is None:
            return None
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _require_ready(self):
        if not self._ready:
            raise capi.GstTacoError(-4, "weights not loaded (call Restore first)")

    # ------------------------------------------------------------------ hot path
    def Inference_Step(self, tokens, token_lengths=None, initial_mels=None, mels_for_gst=None,
                       mel_lengths_for_gst=None, prenet_masks=None, attn_noise=None, seed=None,
                       steps=None, return_pre_mel=False, masked=False, with_vocoder=False, style_embeddings=None,
                       teacher_mels=None, seeds=None):
        """reference Model.py:249-255.  Returns (mel_Logits [B,S*r,mel], stop_Logits [B,S],
        spectrogram_Logits ([B,S*r,Spectrogram_Dim] with ``with_vocoder=True``, else None), alignments [B,S,T_v]) as
        CUDA tensors on the current stream.
        ``masked=True`` (extension): honour ``token_lengths`` so each utterance of a ragged batch equals
        that utterance run alone; the default ignores them like the reference does.
        ``with_vocoder=True`` also runs Vocoder_Taco1 (CBHG) and returns spectrogram_Logits [B,S*r,513]
        as the third element like the reference; the default returns None there (the north-star metric excludes it).
        ``style_embeddings`` (extension) [batch, Style_Token.Attention.Size], or [1, ...] for one style for the whole batch: the
        style is given instead of computed from ``mels_for_gst`` (which must then be None); the reference encoder and the style-token
        layer are skipped, everything downstream is the same code.  With ``Inference_GST_Step``'s output for some mels the results
        are bitwise those of the call with those mels.
        ``teacher_mels`` (extension) [batch, Tq, Mel_Dim] in the reference's ``mels`` layout (Feeder.py:125-139; ``Feeder.Get_Teacher_Pattern``
        builds it): teacher forcing -- step t consumes ``teacher_mels[:, t * r]`` (frame 0 is the go frame, used as given) instead of
        the frame it emitted before, as the reference's training=True loop does (Taco2.py:161,185).  S = ceil((Tq - 1) / r) steps;
        ``steps`` must then be None.  The layers run in inference mode as everywhere here (GTA, not Train_Step's forward), nothing
        is masked by mel length, the same tuple is returned.  Launch path only; one cached graph per distinct S.
        ``seeds`` (extension) [batch] integers, taken mod 2^64, in place of ``seed`` / ``prenet_masks`` / ``attn_noise``: utterance b
        draws the dropout and noise a batch of one draws under ``seed=seeds[b]`` (``Fill_Randomness``, passed on as injected
        randomness).  With ``masked=True`` its outputs are then those of that call alone, whatever its row and the rest of the batch."""
        self._require_ready()
        d = self.dims
        tok = self._dev(tokens, torch.int32)
        if tok.dim() != 2:
            raise ValueError("tokens must be [batch, time]")
        B, Tv = tok.shape
        tlen = None
        if masked:
            if token_lengths is None:
                raise ValueError("masked=True needs token_lengths")
            tlen = self._dev(token_lengths, torch.int32)
            if tuple(tlen.shape) != (B,):
                raise ValueError("token_lengths must be [batch]")
        mels = lens = style = None
        Tref1 = 0
        if style_embeddings is not None:
            if mels_for_gst is not None or mel_lengths_for_gst is not None:
                raise ValueError("style_embeddings and mels_for_gst are mutually exclusive")
            if not d.gst:
                raise ValueError("GST is not used")
            style = self._dev(style_embeddings, torch.float32)
            if style.dim() != 2 or style.shape[0] not in (1, B) or style.shape[1] != d.gst_att:
                raise ValueError("style_embeddings must be [batch, {0}] or [1, {0}]".format(d.gst_att))
            if style.shape[0] != B:
                style = style.expand(B, -1).contiguous()
        elif d.gst:
            if mels_for_gst is None or mel_lengths_for_gst is None:
                raise ValueError("GST is enabled, but no mel information.")
            mels = self._dev(mels_for_gst, torch.float32)
            lens = self._dev(mel_lengths_for_gst, torch.int32)
            if mels.dim() != 3 or mels.shape[0] != B or mels.shape[2] != d.mel or lens.shape != (B,):
                raise ValueError("mels_for_gst must be [batch, frames+1, Mel_Dim] with mel_lengths_for_gst [batch]")
            Tref1 = mels.shape[1]
        teacher, Tq = self._teacher(teacher_mels, B, steps)
        S = (Tq - 1 + d.r - 1) // d.r if teacher is not None else d.steps if steps is None else int(steps)
        if seeds is not None:
            self._seeds_exclusive(seed, prenet_masks, attn_noise)
            prenet_masks, attn_noise = self.Fill_Randomness(seeds, S, Tv, batch=B)
            seed = 0
        masks = self._dev(prenet_masks, torch.float32)
        noise = self._dev(attn_noise, torch.float32)
        if masks is not None and masks.numel() != S * B * sum(d.prenet):
            raise ValueError("prenet_masks must be [steps, 2, batch, prenet]")
        if noise is not None and tuple(noise.shape) != (S, B, Tv):
            raise ValueError("attn_noise must be [steps, batch, T_v]")
        mel = torch.empty((B, S * d.r, d.mel), dtype=torch.float32, device=self.device)
        pre = torch.empty_like(mel) if return_pre_mel else None
        spec = None
        if with_vocoder:
            if not d.vocoder:
                raise ValueError("Hyper_Parameters has no Vocoder_Taco1 section")
            spec = torch.empty((B, S * d.r, d.spec), dtype=torch.float32, device=self.device)
        stop = torch.empty((B, S), dtype=torch.float32, device=self.device)
        align = torch.empty((B, S, Tv), dtype=torch.float32, device=self.device)
        if seed is None:
            self.seed += 1
            seed = self.seed
        with torch.cuda.device(self.device):
            if teacher is not None:
                self.ctx.check(self.ctx.lib.gsttaco_inference_step_forced(
                    self.ctx.handle, _ptr(tok), _ptr(tlen), _ptr(mels), _ptr(lens), _ptr(style), _ptr(masks), _ptr(noise),
                    ctypes.c_uint64(int(seed)), B, Tv, Tref1, _ptr(teacher), Tq, _ptr(mel), _ptr(stop), _ptr(align), _ptr(pre),
                    _ptr(spec), self._stream()))
            elif style is not None:
                self.ctx.check(self.ctx.lib.gsttaco_inference_step_styled(
                    self.ctx.handle, _ptr(tok), _ptr(tlen), _ptr(style), _ptr(masks), _ptr(noise),
                    ctypes.c_uint64(int(seed)), B, Tv, S, _ptr(mel), _ptr(stop), _ptr(align), _ptr(pre), _ptr(spec),
                    self._stream()))
            else:
                self.ctx.check(self.ctx.lib.gsttaco_inference_step(
                    self.ctx.handle, _ptr(tok), _ptr(tlen), _ptr(mels), _ptr(lens), _ptr(masks), _ptr(noise),
                    ctypes.c_uint64(int(seed)), B, Tv, Tref1, S, _ptr(mel), _ptr(stop), _ptr(align), _ptr(pre), _ptr(spec),
                    self._stream()))
        if return_pre_mel:
            return mel, stop, spec, align, pre
        return mel, stop, spec, align

    @staticmethod
    def _seeds_exclusive(seed, prenet_masks, attn_noise):
        if seed is not None or prenet_masks is not None or attn_noise is not None:
            raise ValueError("seeds is mutually exclusive with seed, prenet_masks and attn_noise")

    def Fill_Randomness(self, seeds, steps, Tv, batch=None):
        """Extension: (prenet_masks [steps, 2, B, prenet], attn_noise [steps, B, Tv] -- None unless the attention is SMA) on the device,
        in the layouts ``Inference_Step(prenet_masks=, attn_noise=)`` takes, with row b drawn from ``seeds[b]`` as a batch of one draws
        its row 0 under that seed (``gsttaco_fill_randomness``): independent of B, of the row order and of ``Tv``.  ``seeds`` [B]
        integers, taken mod 2^64.  Works before Restore (no weights involved)."""
        d = self.dims
        if torch.is_tensor(seeds):
            seeds = seeds.cpu().numpy()
        vals = [int(v) & checked.MASK64 for v in np.asarray(seeds, dtype=object).reshape(-1)]
        if np.ndim(seeds) != 1 or not vals or (batch is not None and len(vals) != batch):
            raise ValueError("seeds must be [batch]")
        if not torch.cuda.is_available():
            raise capi.GstTacoError(-2, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)")
        B = len(vals)
        dev_seeds = torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64)).to(self.device)      # (the same 64 bits)
        masks = torch.empty((steps, 2, B, d.prenet[0]), dtype=torch.float32, device=self.device)
        noise = torch.empty((steps, B, Tv), dtype=torch.float32, device=self.device) if d.att_type == "SMA" else None
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_fill_randomness(self.ctx.handle, _ptr(dev_seeds), B, int(Tv), int(steps), _ptr(masks),
                                                                _ptr(noise), self._stream()))
        return masks, noise

    def Utterance_Report(self, stops, alignments, token_lengths=None, mels=None):
        """Extension: the synthesis report of ``stops`` [B, S] and ``alignments`` [B, S, T_v] as ``Inference_Step`` returns them ->
        (report int32 [B, 8], focus float32 [B]) on the device (``gsttaco_utterance_report``).  The columns are ``REPORT_FIELDS``:
        stop_step (== S: the stop token never fired), frames (what ``Inv_Spectrogram(frames=)`` takes), end_gap (> 0: the attention did
        not reach the last token), max_jump, back_steps, max_stall, visited, nonfinite; focus is the mean attention maximum over the
        steps before the stop.  ``token_lengths`` [B] limits each utterance's columns, ``mels`` [B, S * r, Mel_Dim] adds the frames
        before the stop to the non-finite count.  No thresholds are built in: callers compare the fields themselves."""
        d = self.dims
        st = self._dev(stops, torch.float32)
        al = self._dev(alignments, torch.float32)
        if al.dim() != 3 or st.dim() != 2 or tuple(st.shape) != tuple(al.shape[:2]):
            raise ValueError("stops must be [batch, steps] and alignments [batch, steps, T_v]")
        B, S, Tv = al.shape
        tl = self._dev(token_lengths, torch.int32)
        if tl is not None and tuple(tl.shape) != (B,):
            raise ValueError("token_lengths must be [batch]")
        ml = self._dev(mels, torch.float32)
        if ml is not None and tuple(ml.shape) != (B, S * d.r, d.mel):
            raise ValueError("mels must be [batch, steps * Step_Reduction, Mel_Dim]")
        report = torch.empty((B, len(REPORT_FIELDS)), dtype=torch.int32, device=self.device)
        focus = torch.empty((B,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_utterance_report(self.ctx.handle, _ptr(st), _ptr(al), _ptr(tl), _ptr(ml), B, S, Tv,
                                                                 _ptr(report), _ptr(focus), self._stream()))
        return report, focus

    def _teacher(self, teacher_mels, B, steps):
        """(device tensor [B, Tq, Mel_Dim], Tq) of a ``teacher_mels`` argument, or (None, 0)."""
        if teacher_mels is None:
            return None, 0
        if steps is not None:
            raise ValueError("teacher_mels fixes the step count (ceil((Tq - 1) / Step_Reduction)): steps must be None")
        t = self._dev(teacher_mels, torch.float32)
        if t.dim() != 3 or t.shape[0] != B or t.shape[2] != self.dims.mel or t.shape[1] < 2:
            raise ValueError("teacher_mels must be [batch, Tq >= 2, Mel_Dim] (frame 0 = the go frame)")
        return t, int(t.shape[1])

    def Forced_Durations(self, alignments, token_lengths=None, mel_lengths=None):
        """Extension: frames per token of ``alignments`` [B, S, T_v] (as ``Inference_Step`` returns them) -> int32 [B, T_v] on the
        device.  Frame f of utterance b (f < min(mel_lengths[b], S * r); S * r without ``mel_lengths``) counts for token
        argmax_{j < token_lengths[b]} alignments[b, f // r, j] (all T_v columns without ``token_lengths``; the lowest index on a tie):
        rows sum to the length, columns beyond the token length are 0 (``gsttaco_forced_durations``)."""
        al = self._dev(alignments, torch.float32)
        if al.dim() != 3:
            raise ValueError("alignments must be [batch, steps, T_v]")
        B, S, Tv = al.shape
        tl = self._dev(token_lengths, torch.int32)
        ml = self._dev(mel_lengths, torch.int32)
        for name, v in (("token_lengths", tl), ("mel_lengths", ml)):
            if v is not None and tuple(v.shape) != (B,):
                raise ValueError(name + " must be [batch]")
        dur = torch.empty((B, Tv), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_forced_durations(self.ctx.handle, _ptr(al), _ptr(tl), _ptr(ml), B, S, Tv, _ptr(dur),
                                                                 self._stream()))
        return dur

    def Inference_GTA(self, sentence_List, mel_or_wav_List, wav_List_for_GST=None, style_embeddings=None, seeds=None, **kwargs):
        """Extension: ground-truth-aligned (GTA) mels.  ``mel_or_wav_List`` holds one target per sentence: mels [T, Mel_Dim] (as
        Pattern_Generator stores them) or wav paths / 1-D sample arrays, which go through ``Mel_Generate`` (top_db 15, the value
        Feeder.py:209 uses for several wavs).  The decoder is teacher-forced on them (``Inference_Step(teacher_mels=...)``; inference-mode
        layers).  The style comes from ``style_embeddings`` or ``wav_List_for_GST`` when given, else from the target audio itself,
        as the reference's training model takes it (Model.py:206).
        Returns (gta_mels: list of [T_i, Mel_Dim] post-net mels trimmed to each target's length, stops [B, S], alignments
        [B, S, T_v], durations int32 [B, T_v] with each row summing to T_i) after ``synchronize()``.
        ``seeds`` [B]: per-utterance seeds (see ``Inference_Step``); the call then runs masked."""
        print("GTA inference running...")
        if seeds is not None:
            kwargs["seeds"], kwargs["masked"] = seeds, True
        targets = list(mel_or_wav_List)
        if len(targets) != len(sentence_List):
            raise ValueError("mel_or_wav_List must hold one target per sentence")
        if not all(self.feeder._is_mel(m) for m in targets):
            mels, lens = self.Mel_Generate(targets, 15)
            mels, lens = mels.cpu().numpy(), lens.cpu().numpy()
            targets = [mels[i, 1:1 + int(lens[i])] for i in range(len(targets))]
        pattern = self.feeder.Get_Teacher_Pattern(sentence_List, targets)
        mel_lengths = pattern.pop("mel_lengths")
        if self.hp_Dict["GST"]["Use"]:
            if style_embeddings is not None:
                if wav_List_for_GST is not None:
                    raise ValueError("wav_List_for_GST and style_embeddings are mutually exclusive")
                pattern["style_embeddings"] = style_embeddings
            else:
                pattern.update(self.feeder.Get_Inference_GST_Pattern(targets if wav_List_for_GST is None else list(wav_List_for_GST)))
        mel, stop, _, align = self.Inference_Step(**pattern, **kwargs)
        dur = self.Forced_Durations(align, pattern["token_lengths"], mel_lengths)
        self.synchronize()
        return [mel[i, :int(n)] for i, n in enumerate(mel_lengths)], stop, align, dur

    def Loss_Terms(self, pre_mel, mel, stop, teacher_mels, mel_lengths=None, spectrogram=None, spectrogram_targets=None,
                   spectrogram_lengths=None):
        """Extension: the loss sums of a teacher-forced pass (``gsttaco_losses``) -> float64 [B, 6] on the device, columns
        ``LOSS_FIELDS``.  ``pre_mel`` / ``mel`` [B, S * r, Mel_Dim], ``stop`` [B, S] and ``spectrogram`` [B, S * r, Spectrogram_Dim] as
        ``Inference_Step(teacher_mels=, return_pre_mel=True, with_vocoder=True)`` returns them; ``teacher_mels`` [B, Tq, Mel_Dim] and
        ``spectrogram_targets`` [B, Tq, Spectrogram_Dim] with the go frame at index 0: the target of frame t is frame 1 + t.  Per
        utterance: sums over the frames below its length of the channel means of |difference| and difference^2, and the stop token's
        sigmoid cross entropy summed over all steps (label 1 while s < ceil(mel_length / r)).  The spectrogram fields are 0 unless
        both spectrogram tensors are given.  Works before Restore (no weights involved)."""
        d = self.dims
        pm, ml, st = self._dev(pre_mel, torch.float32), self._dev(mel, torch.float32), self._dev(stop, torch.float32)
        tg = self._dev(teacher_mels, torch.float32)
        if st.dim() != 2:
            raise ValueError("stop must be [batch, steps]")
        B, S = st.shape
        if tg.dim() != 3 or tg.shape[0] != B or tg.shape[2] != d.mel or tg.shape[1] < 2:
            raise ValueError("teacher_mels must be [batch, Tq >= 2, Mel_Dim] (frame 0 = the go frame)")
        Tq = int(tg.shape[1])
        if S * d.r < Tq - 1:
            raise ValueError("the predictions hold fewer than Tq - 1 frames")
        for name, v in (("pre_mel", pm), ("mel", ml)):
            if tuple(v.shape) != (B, S * d.r, d.mel):
                raise ValueError(name + " must be [batch, steps * Step_Reduction, Mel_Dim]")
        sp, sg = self._dev(spectrogram, torch.float32), self._dev(spectrogram_targets, torch.float32)
        if sp is not None and tuple(sp.shape) != (B, S * d.r, d.spec):
            raise ValueError("spectrogram must be [batch, steps * Step_Reduction, Spectrogram_Dim]")
        if sg is not None and tuple(sg.shape) != (B, Tq, d.spec):
            raise ValueError("spectrogram_targets must be [batch, Tq, Spectrogram_Dim] with teacher_mels' Tq")
        mlen, slen = self._dev(mel_lengths, torch.int32), self._dev(spectrogram_lengths, torch.int32)
        for name, v in (("mel_lengths", mlen), ("spectrogram_lengths", slen)):
            if v is not None and tuple(v.shape) != (B,):
                raise ValueError(name + " must be [batch]")
        if not torch.cuda.is_available():
            raise capi.GstTacoError(-2, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)")
        sums = torch.empty((B, len(LOSS_FIELDS)), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_losses(self.ctx.handle, _ptr(pm), _ptr(ml), _ptr(st), _ptr(sp), _ptr(tg), _ptr(sg),
                                                       _ptr(mlen), _ptr(slen), B, S, Tq, _ptr(sums), self._stream()))
        return sums

    def Evaluate_Step(self, tokens, token_lengths, teacher_mels, mel_lengths, spectrograms=None, spectrogram_lengths=None,
                      style_embeddings=None, mels_for_gst=None, mel_lengths_for_gst=None, **kwargs):
        """Extension: one teacher-forced ``Inference_Step`` (``return_pre_mel=True``; the vocoder runs iff ``spectrograms`` -- the targets
        [B, Tq, Spectrogram_Dim] -- are given) and ``Loss_Terms`` of its outputs on the same stream.  Returns (sums float64 [B, 6],
        (mel, stop, spec, align, pre_mel)).  ``kwargs``: ``seed`` / ``seeds`` / ``prenet_masks`` / ``attn_noise`` and ``masked`` as
        ``Inference_Step`` takes them.  With GST on and no style given the style input is ``teacher_mels`` itself with ``mel_lengths``
        -- go frame and trailing padding included --, which is what the reference's training model is fed (Model.py:206:
        ``[mels, mel_lengths]``), not ``Inference_GTA``'s re-packed copy.  Every layer runs in inference mode: this is the
        validation loss of the inference graph, not Train_Step's forward (no batch-statistics BN, no encoder dropout)."""
        for k in kwargs:
            if k not in ("seed", "seeds", "prenet_masks", "attn_noise", "masked"):
                raise ValueError("Evaluate_Step sets '{}' itself".format(k))
        if self.dims.gst and style_embeddings is None and mels_for_gst is None:
            mels_for_gst, mel_lengths_for_gst = teacher_mels, mel_lengths
        out = self.Inference_Step(tokens, token_lengths, None, mels_for_gst, mel_lengths_for_gst, return_pre_mel=True,
                                  with_vocoder=spectrograms is not None, style_embeddings=style_embeddings,
                                  teacher_mels=teacher_mels, **kwargs)
        mel, stop, spec, align, pre = out
        sums = self.Loss_Terms(pre, mel, stop, teacher_mels, mel_lengths, spec, spectrograms, spectrogram_lengths)
        return sums, out

    def Evaluate(self, sentence_List, mel_or_wav_List, spectrogram_List=None, use_l2=None, seeds=None, **kwargs):
        """Extension: the loss the reference's ``Train_Step`` computes (Model.py:210-241), as a validation number of this checkpoint on
        the given sentences and targets.  ``mel_or_wav_List`` holds one target per sentence: wav paths / 1-D sample arrays, which go
        through ``Feature_Generate`` (top_db 15, what ``Inference_GTA`` uses) and then carry their spectrogram targets with them, or
        mels [T, Mel_Dim] taken as given, with ``spectrogram_List`` ([T, Spectrogram_Dim] each) optionally beside them.  The
        spectrogram term is included only when spectrogram targets exist (and the model has a vocoder).  ``use_l2``:
        ``Train.Use_L2_Loss``; None reads it from the hyper parameters (False when absent).
        Returns a dict: ``pre_mel``, ``mel``, ``stop``, ``spectrogram``, ``loss`` (``evaluate.combine``: means over the PADDED batch like
        the reference's, so padding dilutes the frame terms), ``per_utterance`` (numpy float64 [B, 6], ``LOSS_FIELDS``: sums),
        ``mel_lengths`` and ``steps``.
        Prenet dropout and the SMA noise are live at inference, so these losses are random variables: give ``seed`` or ``seeds``
        ([B], per utterance; the call then runs masked) for a repeatable number."""
        print("Evaluation running...")
        if seeds is not None:
            kwargs["seeds"], kwargs["masked"] = seeds, True
        targets = list(mel_or_wav_List)
        if len(targets) != len(sentence_List):
            raise ValueError("mel_or_wav_List must hold one target per sentence")
        if not all(self.feeder._is_mel(m) for m in targets):
            if spectrogram_List is not None:
                raise ValueError("wav targets bring their own spectrograms: spectrogram_List must be None")
            mels, specs, lens = self.Feature_Generate(targets, 15)
            mels, specs, lens = mels.cpu().numpy(), specs.cpu().numpy(), lens.cpu().numpy()
            targets = [mels[i, 1:1 + int(lens[i])] for i in range(len(targets))]
            if self.dims.vocoder:
                spectrogram_List = [specs[i, 1:1 + int(lens[i])] for i in range(len(targets))]
        pattern = self.feeder.Get_Evaluation_Pattern(sentence_List, targets, spectrogram_List)
        sums, out = self.Evaluate_Step(**pattern, **kwargs)
        self.synchronize()
        per = sums.cpu().numpy()
        S, T = int(out[1].shape[1]), int(pattern["teacher_mels"].shape[1]) - 1
        result = evaluate.combine(per, T, S, evaluate.use_l2_of(self.hp_Dict) if use_l2 is None else bool(use_l2))
        result.update(per_utterance=per, mel_lengths=pattern["mel_lengths"], steps=S)
        return result

    def _frames_view(self, t, name):
        """A float32 device tensor [B, T, Mel_Dim] whose frames are dense (a slice along the frame axis stays a view: its batch stride is
        passed on), the batch stride in floats and T."""
        t = t if isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == torch.float32 else self._dev(t, torch.float32)
        if t.dim() != 3 or t.shape[2] != self.dims.mel or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(name + " must be [batch, frames >= 1, Mel_Dim]")
        if t.stride(2) != 1 or t.stride(1) != t.shape[2] or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * t.shape[2]):
            t = t.contiguous()
        return t, int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1] * t.shape[2]), int(t.shape[1])

    def Mel_DTW(self, mels, mel_lengths, ref_mels, ref_lengths, n_ceps=13, return_path=False):
        """Extension: mel-cepstral distortion along a dynamic-time-warping path (``gsttaco_mel_dtw``) between ``mels`` [B, Tx, Mel_Dim]
        (synthesised) and ``ref_mels`` [B, Ty, Mel_Dim] (reference), torch or numpy, with ``mel_lengths`` / ``ref_lengths`` [B] or None
        (all frames; ``mel_lengths`` may be the ``frames`` column of ``Utterance_Report`` as a device tensor).  A view sliced along the
        frame axis -- ``mels_for_gst[:, 1:]`` -- is taken without a copy.  Returns (cost float64 [B], path_len int32 [B]) on the
        device, and with ``return_path=True`` also path int32 [B, Tx + Ty - 1, 2]: the cells (i, j) from (0, 0) to the last frames,
        -1 beyond ``path_len``.  ``cost / path_len`` is the utterance's MCD in dB of the log-mel cepstra 1 .. ``n_ceps`` (0: the mel
        channels themselves); comparable between checkpoints of one configuration, not with SPTK mel-cepstrum figures.  Works before
        Restore (no weights involved)."""
        x, xs, Tx = self._frames_view(mels, "mels")
        y, ys, Ty = self._frames_view(ref_mels, "ref_mels")
        B = int(x.shape[0])
        if y.shape[0] != B:
            raise ValueError("mels and ref_mels must have one batch size")
        xl, yl = self._dev(mel_lengths, torch.int32), self._dev(ref_lengths, torch.int32)
        for name, v in (("mel_lengths", xl), ("ref_lengths", yl)):
            if v is not None and tuple(v.shape) != (B,):
                raise ValueError(name + " must be [batch]")
        if not torch.cuda.is_available():
            raise capi.GstTacoError(-2, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)")
        cost = torch.empty((B,), dtype=torch.float64, device=self.device)
        plen = torch.empty((B,), dtype=torch.int32, device=self.device)
        path = torch.empty((B, Tx + Ty - 1, 2), dtype=torch.int32, device=self.device) if return_path else None
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_mel_dtw(self.ctx.handle, _ptr(x), _ptr(xl), xs, _ptr(y), _ptr(yl), ys, B, Tx, Ty, int(n_ceps),
                                                        _ptr(cost), _ptr(plen), _ptr(path), self._stream()))
        return (cost, plen, path) if return_path else (cost, plen)

    def Evaluate_Free(self, sentence_List, mel_or_wav_List, wav_List_for_GST=None, style_embeddings=None, seeds=None, n_ceps=13,
                      pitch=False, **kwargs):
        """Extension: the free-run metric of this checkpoint on the given sentences and targets -- what ``Evaluate`` cannot give, because
        the free-running decoder's output has another length than its target: one ``Inference_Step`` (not teacher-forced),
        ``Utterance_Report`` for the frames each utterance used, and ``Mel_DTW`` of those frames against the target's.
        ``mel_or_wav_List`` holds one target per sentence as ``Evaluate`` takes them: wav paths / 1-D sample arrays (``Mel_Generate`` at
        top_db 15) or mels [T, Mel_Dim] taken as given.  The style comes from ``style_embeddings`` or ``wav_List_for_GST`` when given,
        else from the target itself.  ``seeds`` [B]: per-utterance seeds; the call then runs masked (dropout is live at inference:
        without a seed the number is a random variable).  ``kwargs`` go to ``Inference_Step`` (``seed``, ``steps``, ``masked``, ...).
        Nothing is read back before the final result.  Returns a dict: ``mcd`` (the mean over utterances of cost / path_len, dB),
        ``mcd_frames`` (sum cost / sum path_len), ``per_utterance`` (numpy float64 [B, 7], ``evaluate.FREE_FIELDS``), ``report`` (numpy
        int32 [B, 8], ``REPORT_FIELDS``), ``mel_lengths`` / ``ref_lengths`` (numpy int32 [B]), and the device tensors ``mels``
        [B, S * r, Mel_Dim] and ``ref_mels`` [B, T, Mel_Dim] the distance was taken between.
        ``pitch=True`` (or a dict of the tracker's ``fmin`` / ``fmax`` / ``threshold`` / ``window``, applied to both sides, in place
        of ``Pitch``'s defaults) adds the prosody metrics (the targets must then be wavs): the targets are staged once and both their mel and
        their F0 (``Pitch_Signals`` at the same top_db 15) come from that batch; the step also runs the vocoder, ``Inv_Spectrogram``
        turns the report's ``frames`` of its spectrogram into a waveform (Griffin-Lim under the seed ``seeds[0]`` / ``seed`` / the
        model's counter plus 0x9E3779B97F4A7C15, mod 2^64), ``Pitch_Signals`` tracks it untrimmed, and ``Pitch_Errors`` compares the two
        tracks along the DTW path.  The synthesised side's F0 is therefore that of the Griffin-Lim waveform of the vocoder's
        spectrogram: comparable between checkpoints and styles of one configuration, not with figures taken off another vocoder.  The
        result gains ``gpe``, ``vde``, ``ffe`` (means over utterances) and ``gpe_frames`` / ``vde_frames`` / ``ffe_frames`` (of the
        pooled counts; ``evaluate.summarize_pitch``), ``pitch_per_utterance`` (numpy float64 [B, 8], ``evaluate.PITCH_FIELDS``) and the
        device tensors ``f0`` [B, S * r] and ``ref_f0`` [B, >= T].  Without the flag nothing of this runs."""
        print("Free-run evaluation running...")
        for k in ("teacher_mels", "return_pre_mel", "with_vocoder", "mels_for_gst", "mel_lengths_for_gst"):
            if k in kwargs:
                raise ValueError("Evaluate_Free sets '{}' itself".format(k))
        if seeds is not None:
            kwargs["seeds"], kwargs["masked"] = seeds, True
        targets = list(mel_or_wav_List)
        if len(targets) != len(sentence_List):
            raise ValueError("mel_or_wav_List must hold one target per sentence")
        track = dict(pitch) if isinstance(pitch, dict) else {}
        pitch = bool(pitch) or isinstance(pitch, dict)
        if pitch:
            if any(k not in ("fmin", "fmax", "threshold", "window") for k in track):
                raise ValueError("pitch takes True or a dict of fmin / fmax / threshold / window")
            if any(self.feeder._is_mel(m) for m in targets):
                raise ValueError("pitch=True needs wav targets: a mel does not carry its F0")
            if not self.dims.vocoder:
                raise ValueError("pitch=True needs the vocoder: Hyper_Parameters has no Vocoder_Taco1 section")
            base = seeds[0] if seeds is not None else kwargs["seed"] if kwargs.get("seed") is not None else self.seed + 1
            gl_seed = (int(base) + 0x9E3779B97F4A7C15) & checked.MASK64
            staged = self._stage_wavs(targets)
            ref_all, ref_len = self._mel_of_staged(*staged, 15)
            ref_f0, _, ref_f0_len = self.Pitch_Signals(staged[0], staged[1], 15, **track)
        elif all(self.feeder._is_mel(m) for m in targets):
            ref = self.feeder.Get_Inference_GST_Pattern(targets)
            ref_all, ref_len = self._dev(ref["mels_for_gst"], torch.float32), self._dev(ref["mel_lengths_for_gst"], torch.int32)
        else:
            ref_all, ref_len = self.Mel_Generate(targets, 15)
        pattern = self.feeder.Get_Inference_Pattern(sentence_List, style_given=True)
        if self.hp_Dict["GST"]["Use"]:
            if style_embeddings is not None:
                if wav_List_for_GST is not None:
                    raise ValueError("wav_List_for_GST and style_embeddings are mutually exclusive")
                pattern["style_embeddings"] = style_embeddings
            elif wav_List_for_GST is not None:
                pattern.update(self.feeder.Get_Inference_GST_Pattern(list(wav_List_for_GST)))
            else:
                pattern["mels_for_gst"], pattern["mel_lengths_for_gst"] = ref_all, ref_len
        mel, stop, spec, align = self.Inference_Step(**pattern, with_vocoder=pitch, **kwargs)
        report, _ = self.Utterance_Report(stop, align, pattern["token_lengths"] if kwargs.get("masked") else None, mel)
        frames = report[:, REPORT_FIELDS.index("frames")].contiguous()
        ref_mels = ref_all[:, 1:]                                   # (behind the prepended zero frame: a view, no copy)
        if pitch:
            syn_wav, syn_len = self.Inv_Spectrogram(spec, frames=frames, seed=gl_seed)
            f0, _, f0_len = self.Pitch_Signals(syn_wav, syn_len, **track)
            cost, plen, path = self.Mel_DTW(mel, frames, ref_mels, ref_len, n_ceps=n_ceps, return_path=True)
            counts, sums = self.Pitch_Errors(f0, f0_len, ref_f0, ref_f0_len, path, plen)
        else:
            cost, plen = self.Mel_DTW(mel, frames, ref_mels, ref_len, n_ceps=n_ceps)
        self.synchronize()
        rep, ref_lengths = report.cpu().numpy(), ref_len.cpu().numpy()
        per = evaluate.combine_free(cost.cpu().numpy(), plen.cpu().numpy(), rep[:, 1], ref_lengths, rep[:, 0], int(stop.shape[1]))
        result = evaluate.summarize_free(per)
        result.update(per_utterance=per, report=rep, mel_lengths=rep[:, 1].copy(), ref_lengths=ref_lengths, mels=mel, ref_mels=ref_mels)
        if pitch:
            counts, sums = counts.cpu().numpy(), sums.cpu().numpy()
            result.update(evaluate.summarize_pitch(counts, sums))
            result.update(pitch_per_utterance=evaluate.combine_pitch(counts, sums), f0=f0, ref_f0=ref_f0)
        return result

    def Inference_GST(self, wav_List, tag_List=None, label=None, style_map=False):
        """reference Model.py:427-446: style embeddings [B, Attention.Size] of the wavs; with ``tag_List`` the table
        of Model.py:448-459 is written too.  ``style_map`` (extension; True or a dict of ``Style_Map`` keywords): the embeddings go
        on to ``Style_Map`` without leaving the device and the method returns (gsts, map dict); with ``tag_List`` the map is written
        beside the table as GST/<label>.GST.MAP.TXT and, where matplotlib imports, drawn as GST/<label>.GST.PNG -- the figure
        reference R_Script/TSNE.R makes of the table."""
        if not self.hp_Dict["GST"]["Use"]:
            raise NotImplementedError("GST is not used")
        print("GST Inference running...")
        gsts = self.Inference_GST_Step(**self.feeder.Get_Inference_GST_Pattern(wav_List))
        label = label or datetime.now().strftime("%Y%m%d.%H%M%S")
        if tag_List is not None:
            self.Export_GST(wav_List, tag_List, gsts, label)
        if style_map is False or style_map is None:
            return gsts
        result = self.Style_Map(gsts, **({} if style_map is True else dict(style_map)))
        if tag_List is not None:
            self.Export_GST_Map(wav_List, tag_List, result["y"], label)
        return gsts, result

    def Style_Affinities(self, embeddings, perplexity=5.0):
        """Extension: the symmetric affinities of exact t-SNE (``gsttaco_style_affinities``) over ``embeddings`` [N, D] -- what
        ``Inference_GST_Step`` returns, or any float array; a device tensor whose rows are dense is read where it lies.  Returns
        (p float64 [N, N], beta float64 [N], search_iters int32 [N]) on the device.  ``perplexity`` lies in (1, N - 1).  The affinities
        do not depend on the embeddings' scale: every point's bandwidth is searched for.  Works before Restore."""
        if not torch.cuda.is_available():
            raise capi.GstTacoError(-2, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)")
        x = embeddings
        if not (isinstance(x, torch.Tensor) and x.device == self.device and x.dtype == torch.float32 and x.dim() == 2
                and x.stride(1) == 1 and x.stride(0) >= x.shape[1]):
            x = self._dev(x, torch.float32)
        if x.dim() != 2:
            raise ValueError("embeddings must be [points, channels]")
        N, D = int(x.shape[0]), int(x.shape[1])
        p = torch.empty((N, N), dtype=torch.float64, device=self.device)
        beta = torch.empty((N,), dtype=torch.float64, device=self.device)
        rounds = torch.empty((N,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_style_affinities(self.ctx.handle, _ptr(x), N, D, int(x.stride(0)), float(perplexity), _ptr(p),
                                                                 _ptr(beta), _ptr(rounds), self._stream()))
        return p, beta, rounds

    def Style_Map(self, embeddings=None, affinities=None, perplexity=5.0, iters=1000, seed=0, init=None, state=None, exaggeration=12.0,
                  stop_lying_iter=250, mom_switch_iter=250, momentum=0.5, final_momentum=0.8, eta=200.0):
        """Extension: the style map -- exact (theta = 0) t-SNE of style embeddings into two dimensions on the device
        (``gsttaco_style_map``), with the defaults of reference R_Script/TSNE.R and Rtsne (perplexity 5, 1000 iterations).  Exactly one
        of ``embeddings`` [N, D] (``Style_Affinities`` runs first) and ``affinities`` [N, N] float64 is given; with ``state`` -- a
        previous result -- neither need be: the state's own affinities are used and the descent continues at its ``iter`` for ``iters``
        more steps, bitwise as one longer run would.  The map starts at ``init`` [N, 2], by default ``style_map_init(N, seed)``: drawn
        on the host.  Returns a dict: ``y`` [N, 2], ``velocity``, ``gains`` (float64, on the device), ``iter``, ``kl`` (the KL
        divergence at ``y``, a float64 device scalar), ``affinities`` and ``beta`` (None where the affinities were given).
        Not Rtsne's picture point for point: TSNE.R runs the Barnes-Hut form (theta = 0.5) after a PCA to 50 dimensions, this is the
        exact form on all D channels, and a t-SNE map depends on its seed.  Works before Restore."""
        if embeddings is not None and affinities is not None:
            raise ValueError("give embeddings or affinities, not both")
        if not torch.cuda.is_available():
            raise capi.GstTacoError(-2, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)")
        beta = None
        if embeddings is not None:
            affinities, beta, _ = self.Style_Affinities(embeddings, perplexity)
        elif affinities is None:
            if state is None:
                raise ValueError("give embeddings or affinities (or a state, whose affinities are then used)")
            affinities, beta = state["affinities"], state.get("beta")
        elif state is not None and affinities is state.get("affinities"):
            beta = state.get("beta")
        p = self._dev(affinities, torch.float64)
        if p.dim() != 2 or p.shape[0] != p.shape[1]:
            raise ValueError("affinities must be [N, N]")
        N = int(p.shape[0])
        if state is not None:
            if init is not None:
                raise ValueError("give init or state, not both")
            y, velocity, gains = (self._dev(state[k], torch.float64).clone() for k in ("y", "velocity", "gains"))
            first = int(state["iter"])
        else:
            y = self._dev(style_map_init(N, seed) if init is None else np.asarray(init.cpu() if torch.is_tensor(init) else init, dtype=np.float64),
                          torch.float64)
            velocity = torch.zeros((N, 2), dtype=torch.float64, device=self.device)
            gains = torch.ones((N, 2), dtype=torch.float64, device=self.device)
            first = 0
        for name, t in (("init / state y", y), ("velocity", velocity), ("gains", gains)):
            if tuple(t.shape) != (N, 2):
                raise ValueError(name + " must be [N, 2]")
        kl = torch.empty((), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_style_map(self.ctx.handle, _ptr(p), N, _ptr(y), _ptr(velocity), _ptr(gains), first, int(iters),
                                                          float(exaggeration), int(stop_lying_iter), int(mom_switch_iter), float(momentum),
                                                          float(final_momentum), float(eta), _ptr(kl), self._stream()))
        return dict(y=y, velocity=velocity, gains=gains, iter=first + int(iters), kl=kl, affinities=p, beta=beta)

    def Inference_GST_Step(self, mels_for_gst, mel_lengths_for_gst, return_attention=False):
        """reference Model.py:257-265.  ``return_attention=True`` (extension): returns (gst, style_token_weights [B, Head, Style_Token.Size],
        style_query [B, Attention.Size]) -- each head's softmax weights over the tokens and the projected query of the residual, which
        the reference computes and drops (GST.py:105).  ``Style_Compose(style_token_weights, style_query)`` gives ``gst`` back."""
        if not self.hp_Dict["GST"]["Use"]:
            raise NotImplementedError("GST is not used")
        self._require_ready()
        d = self.dims
        mels = self._dev(mels_for_gst, torch.float32)
        lens = self._dev(mel_lengths_for_gst, torch.int32)
        B, Tref1 = mels.shape[0], mels.shape[1]
        gst = torch.empty((B, d.gst_att), dtype=torch.float32, device=self.device)
        if not return_attention:
            with torch.cuda.device(self.device):
                self.ctx.check(self.ctx.lib.gsttaco_gst(self.ctx.handle, _ptr(mels), _ptr(lens), B, Tref1, _ptr(gst), self._stream()))
            return gst
        tw = torch.empty((B, d.heads, d.n_tokens), dtype=torch.float32, device=self.device)
        query = torch.empty((B, d.gst_att), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_gst_ex(self.ctx.handle, _ptr(mels), _ptr(lens), B, Tref1, _ptr(gst), _ptr(tw), _ptr(query),
                                                       self._stream()))
        return gst, tw, query

    def Style_Compose(self, token_weights, query=None):
        """Extension (no reference counterpart): the style embedding [B, Attention.Size] of given token weights,
        LayerNorm(concat_h(token_weights[b, h, :] . V[:, h-slice]) + query) with V = tanh(tokens).Wv + bv -- the last stage of the
        style-token layer (Layers.py:207-211) with the attention weights chosen by the caller.  ``token_weights`` [B, Head,
        Style_Token.Size] are any real numbers: not normalised, not clipped.  ``query`` [B, Attention.Size] is the residual term, None = 0.
        Conditioning on tokens alone (no query) is outside the training distribution of this architecture -- the decoder only ever
        saw LayerNorm(attention output + query) -- but well defined; all-zero weights with no query give exactly the LayerNorm's beta."""
        if not self.hp_Dict["GST"]["Use"]:
            raise NotImplementedError("GST is not used")
        self._require_ready()
        d = self.dims
        tw = self._dev(token_weights, torch.float32)
        if tw.dim() != 3 or tuple(tw.shape[1:]) != (d.heads, d.n_tokens):
            raise ValueError("token_weights must be [batch, {}, {}]".format(d.heads, d.n_tokens))
        B = tw.shape[0]
        q = self._dev(query, torch.float32)
        if q is not None and tuple(q.shape) != (B, d.gst_att):
            raise ValueError("query must be [batch, {}]".format(d.gst_att))
        gst = torch.empty((B, d.gst_att), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_style_compose(self.ctx.handle, _ptr(tw), _ptr(q), B, _ptr(gst), self._stream()))
        return gst

    def _require_audio(self):
        if not self.dims.audio or not self.ctx.cfg.max_wav_samples:
            raise ValueError("the audio front end needs the Sound section of Hyper_Parameters and max_wav_seconds > 0")
        if not torch.cuda.is_available():
            raise capi.GstTacoError(-2, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)")

    @staticmethod
    def _pad_rows(sigs):
        host = np.zeros((len(sigs), max(max(s.shape[0] for s in sigs), 1)), dtype=np.float32)
        for i, s_ in enumerate(sigs):
            host[i, :s_.shape[0]] = s_
        return host

    def Resample(self, signals, rates, target_rate=None):
        """Extension: ``librosa.core.load``'s 'kaiser_best' resampling (``audio.resample_kaiser_best``) of a batch of 1-D sample
        arrays at ``rates`` (one rate, or one per signal) to ``target_rate`` (default Sound.Sample_Rate) on the device
        (gsttaco_resample) -> (device float32 [B, ld] zero-padded, numpy int32 lengths [B] = ceil(n * ratio)): the padded batch the
        front end takes.  A row already at the target rate is copied through.  Works before Restore."""
        self._require_audio()
        target = int(self.dims.sample_rate if target_rate is None else target_rate)
        sigs = [np.asarray(s_, dtype=np.float32) for s_ in signals]
        if not sigs or any(s_.ndim != 1 for s_ in sigs):
            raise ValueError("signals must be a non-empty list of 1-D sample arrays")
        rates = np.broadcast_to(np.asarray(rates, dtype=np.int32), (len(sigs),)).copy()
        return self._resample_rows(sigs, rates, target)

    def _resample_rows(self, sigs, rates, target):
        from .audio import resample_lengths
        B = len(sigs)
        in_len = np.array([s_.shape[0] for s_ in sigs], dtype=np.int32)
        rates = np.ascontiguousarray(rates, dtype=np.int32)
        if (rates < 1).any():
            raise ValueError("a sample rate is not positive")
        ld_out = max(max(resample_lengths(int(n), int(r), target)[1] for n, r in zip(in_len, rates)), 1)
        x = torch.from_numpy(self._pad_rows(sigs)).to(self.device)
        y = torch.empty((B, ld_out), dtype=torch.float32, device=self.device)
        out_len = np.zeros((B,), dtype=np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_resample(
                self.ctx.handle, _ptr(x), in_len.ctypes.data_as(i32p), rates.ctypes.data_as(i32p), B, x.shape[1], target, _ptr(y), ld_out,
                out_len.ctypes.data_as(i32p), self._stream()))
        return y, out_len

    def _stage_wavs(self, wav_List):
        """What both generators feed the front end: (device float32 [B, ld] zero-padded signals at Sound.Sample_Rate, device int32
        lengths [B], B, ld).  An item is a wav path (at any rate), a 1-D sample array already at Sound.Sample_Rate, or a
        ``(samples, rate)`` pair.  Audio at another rate is resampled on the device (``Resample``) and stays there, or with
        ``resample="host"`` by ``audio.resample_kaiser_best`` before the upload; when every item is at the rate already, neither runs."""
        from .audio import as_signal_at_rate, resample_kaiser_best
        self._require_audio()
        target = self.dims.sample_rate
        pairs = [as_signal_at_rate(w, target) for w in wav_List]
        sigs, rates = [p[0] for p in pairs], np.array([p[1] for p in pairs], dtype=np.int32)
        if self.resample == "host":
            sigs = [s_ if r == target else resample_kaiser_best(s_, int(r), target) for s_, r in zip(sigs, rates)]
            rates[:] = target
        if (rates == target).all():
            wav = torch.from_numpy(self._pad_rows(sigs)).to(self.device)
            lens = torch.tensor([s_.shape[0] for s_ in sigs], dtype=torch.int32, device=self.device)
        else:
            wav, out_len = self._resample_rows(sigs, rates, target)
            lens = torch.from_numpy(out_len).to(self.device)
        return wav, lens, wav.shape[0], wav.shape[1]

    def Mel_Generate(self, wav_List, top_db=60):
        """Batched reference Pattern_Generator.Mel_Generate(path, top_db, range_Ignore=True) (Pattern_Generator.py:39-60)
        on the GPU, already in the mels_for_gst layout of Feeder.py:204-225: returns (mels_for_gst [B, 1+max_len, Mel_Dim]
        with a zero frame 0 and zero padding, mel_lengths_for_gst [B]) as device tensors.  ``wav_List`` holds wav paths (at any
        rate), 1-D float sample arrays at Sound.Sample_Rate, or ``(samples, rate)`` pairs; audio at another rate is resampled on
        the device (``Resample``) unless the model was built with ``resample="host"``.  Works before Restore (no weights involved)."""
        return self._mel_of_staged(*self._stage_wavs(wav_List), top_db)

    def _mel_of_staged(self, wav, lens, B, ld, top_db):
        """``Mel_Generate`` of a batch ``_stage_wavs`` has staged (``Evaluate_Free(pitch=True)`` reads the target F0 off the same batch)."""
        d = self.dims
        cap = 2 + ld // d.frame_shift
        mels = torch.empty((B, cap, d.mel), dtype=torch.float32, device=self.device)
        mel_len = torch.empty((B,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_mel_frontend(
                self.ctx.handle, _ptr(wav), _ptr(lens), B, ld, ctypes.c_float(float(top_db)), _ptr(mels), _ptr(mel_len), cap,
                self._stream()))
        n = int(mel_len.max().item())            # the one host sync: the output length is data dependent (trim)
        if int(mel_len.min().item()) < 1:
            raise ValueError("a reference wav is shorter than n_fft/2 samples after trimming (librosa.stft raises there)")
        return mels[:, :n + 1].contiguous(), mel_len

    def Pitch(self, wav_List, top_db=None, fmin=50.0, fmax=500.0, threshold=0.1, window=0):
        """Extension: F0 by YIN (``gsttaco_pitch``) of what ``Mel_Generate`` takes -- wav paths at any rate, 1-D sample arrays at
        Sound.Sample_Rate or ``(samples, rate)`` pairs, staged like there, so other-rate audio is resampled on the device -- on the mel
        front end's frame grid.  ``top_db``: None = no trim; a number = the rows are first cut as ``Mel_Generate(wav_List, top_db)``
        cuts them, and frame t is then frame t of that mel.  Returns (f0 float32 [B, n] in Hz with 0 = unvoiced, aperiodicity float32
        [B, n], frames int32 [B]) as device tensors, cut to the longest row's n frames (one host sync, like ``Mel_Generate``).
        ``fmin`` / ``fmax`` bound the search (lags floor(sr / fmax) .. ceil(sr / fmin)), ``threshold`` is YIN's on the cumulative mean
        normalised difference, ``window`` the integration window in samples (0: 25 ms).  Works before Restore."""
        wav, lens, _, _ = self._stage_wavs(wav_List)
        f0, ap, frames = self.Pitch_Signals(wav, lens, top_db, fmin, fmax, threshold, window)
        n = max(int(frames.max().item()), 1)
        return f0[:, :n].contiguous(), ap[:, :n].contiguous(), frames

    def Pitch_Signals(self, wav, wav_lengths, top_db=None, fmin=50.0, fmax=500.0, threshold=0.1, window=0):
        """Extension: ``Pitch`` of a batch that is on the device already -- ``wav`` float32 [B, ld] at Sound.Sample_Rate with
        ``wav_lengths`` [B], such as ``Inv_Spectrogram`` returns (whose row of k frames gives k F0 frames).  Nothing is read back:
        returns (f0 [B, 1 + ld // Frame_Shift], aperiodicity likewise, frames int32 [B]) uncut; entries beyond a row's frames are 0."""
        self._require_audio()
        d = self.dims
        wav, lens = self._dev(wav, torch.float32), self._dev(wav_lengths, torch.int32)
        if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1 or tuple(lens.shape) != (wav.shape[0],):
            raise ValueError("wav must be [batch, samples] with wav_lengths [batch]")
        B, ld = int(wav.shape[0]), int(wav.shape[1])
        cap = 1 + ld // d.frame_shift
        f0 = torch.empty((B, cap), dtype=torch.float32, device=self.device)
        ap = torch.empty((B, cap), dtype=torch.float32, device=self.device)
        frames = torch.empty((B,), dtype=torch.int32, device=self.device)
        cf = ctypes.c_float
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_pitch(
                self.ctx.handle, _ptr(wav), _ptr(lens), B, ld, cf(-1.0 if top_db is None else float(top_db)), cf(float(fmin)),
                cf(float(fmax)), cf(float(threshold)), int(window), _ptr(f0), _ptr(ap), _ptr(frames), cap, self._stream()))
        return f0, ap, frames

    def Pitch_Errors(self, f0, lengths, ref_f0, ref_lengths, path=None, path_len=None, gross=0.2):
        """Extension: the counts behind gross pitch error, voicing decision error and F0 frame error (``gsttaco_pitch_errors``) of
        ``f0`` [B, Tx] (synthesised) against ``ref_f0`` [B, Ty] (reference), ``lengths`` / ``ref_lengths`` [B] or None (all frames),
        along ``path`` [B, rows, 2] with ``path_len`` [B] as ``Mel_DTW(..., return_path=True)`` returns them -- or, with no path, frame
        i against frame i up to the shorter length (the teacher-forced case).  A frame is voiced where its f0 > 0; a both-voiced pair
        is gross where |f0 - ref_f0| > ``gross`` * ref_f0.  Returns (counts int32 [B, 6], ``evaluate.PITCH_COUNTS``; sums float64
        [B, 2]: sum |c| and sum c^2 of c = 1200 log2(f0 / ref_f0) over the both-voiced non-gross pairs) on the device;
        ``evaluate.combine_pitch`` makes the ratios of them.  Works before Restore."""
        x, y = self._dev(f0, torch.float32), self._dev(ref_f0, torch.float32)
        if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0] or x.shape[0] < 1 or x.shape[1] < 1 or y.shape[1] < 1:
            raise ValueError("f0 and ref_f0 must be [batch, frames >= 1] with one batch size")
        B = int(x.shape[0])
        xl, yl = self._dev(lengths, torch.int32), self._dev(ref_lengths, torch.int32)
        p, pl = self._dev(path, torch.int32), self._dev(path_len, torch.int32)
        for name, v in (("lengths", xl), ("ref_lengths", yl), ("path_len", pl)):
            if v is not None and tuple(v.shape) != (B,):
                raise ValueError(name + " must be [batch]")
        if (p is None) != (pl is None) or (p is not None and (p.dim() != 3 or p.shape[0] != B or p.shape[1] < 1 or p.shape[2] != 2)):
            raise ValueError("path must be [batch, rows, 2] and come with path_len [batch]")
        if not torch.cuda.is_available():
            raise capi.GstTacoError(-2, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)")
        counts = torch.empty((B, len(evaluate.PITCH_COUNTS)), dtype=torch.int32, device=self.device)
        sums = torch.empty((B, 2), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_pitch_errors(
                self.ctx.handle, _ptr(x), _ptr(xl), int(x.shape[1]), _ptr(y), _ptr(yl), int(y.shape[1]), _ptr(p), _ptr(pl),
                int(p.shape[1]) if p is not None else 0, B, ctypes.c_float(float(gross)), _ptr(counts), _ptr(sums), self._stream()))
        return counts, sums

    def Feature_Generate(self, wav_List, top_db=60):
        """Extension: ``Mel_Generate`` plus the linear spectrogram of the same trimmed signal from the same STFT (reference
        Pattern_Generator.Spectrogram_Generate / Audio.spectrogram, Audio.py:18-21: what Train_Step compares the vocoder's output
        with) -> (mels [B, 1+max_len, Mel_Dim], spectrograms [B, 1+max_len, Spectrogram_Dim], lengths [B]) as device tensors, both
        with a zero frame 0 and zero padding.  ``mels`` is bitwise ``Mel_Generate``'s.  Works before Restore."""
        d = self.dims
        wav, lens, B, ld = self._stage_wavs(wav_List)
        cap = 2 + ld // d.frame_shift
        mels = torch.empty((B, cap, d.mel), dtype=torch.float32, device=self.device)
        specs = torch.empty((B, cap, d.spec), dtype=torch.float32, device=self.device)
        out_len = torch.empty((B,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_feature_frontend(
                self.ctx.handle, _ptr(wav), _ptr(lens), B, ld, ctypes.c_float(float(top_db)), _ptr(mels), _ptr(specs), _ptr(out_len),
                cap, self._stream()))
        n = int(out_len.max().item())            # the one host sync: the output length is data dependent (trim)
        if int(out_len.min().item()) < 1:
            raise ValueError("a wav is shorter than n_fft/2 samples after trimming (librosa.stft raises there)")
        return mels[:, :n + 1].contiguous(), specs[:, :n + 1].contiguous(), out_len

    def Inference(self, sentence_List, wav_List_for_GST=None, label=None, export=False, style_embeddings=None,
                  style_token_weights=None, seeds=None, vocoder="griffin_lim", **kwargs):
        """reference Model.py:342-367.  ``wav_List_for_GST`` holds wav paths / 1-D sample arrays like the reference's,
        or precomputed mels [T, Mel_Dim].  The reference always starts its export thread; here ``export=True`` asks for
        it (it needs the CBHG vocoder and Griffin-Lim, which are off the mel-frame metric) and runs it synchronously.
        Extension: instead of reference audio, ``style_embeddings`` [B, A] / [1, A] (see ``Inference_Step``) or
        ``style_token_weights`` [Head, Style_Token.Size], [1, Head, Size] or [B, Head, Size] -- composed with no query
        (``Style_Compose``: outside the training distribution, see there) and then used as embeddings.
        ``seeds`` [B] (extension): per-utterance seeds (see ``Inference_Step``); the call then runs with ``masked=True`` -- without
        masking the batch's padding reaches every utterance, which is what the seeds exist to rule out.
        ``vocoder`` (extension): what ``export=True`` makes the WAVs with -- "griffin_lim" (the reference's, the default), "melgan"
        (``Load_Neural_Vocoder`` first), "waveglow" (``Load_WaveGlow`` first; an utterance's decode seed is also its vocoder seed,
        without ``seeds`` every row's is 0) or "hifigan" (``Load_HiFiGAN`` first); see ``Export_Inference``."""
        self._check_vocoder(vocoder)
        print("Inference running...")
        if seeds is not None:
            kwargs["seeds"], kwargs["masked"] = seeds, True
        styled = style_embeddings is not None or style_token_weights is not None
        if styled:
            if wav_List_for_GST is not None or (style_embeddings is not None and style_token_weights is not None):
                raise ValueError("wav_List_for_GST, style_embeddings and style_token_weights are mutually exclusive")
            if not self.hp_Dict["GST"]["Use"]:
                raise ValueError("GST is not used")
            if style_token_weights is not None:
                tw = self._dev(style_token_weights, torch.float32)
                if tw.dim() == 2:
                    tw = tw.unsqueeze(0)
                if tw.dim() != 3 or tw.shape[0] not in (1, len(sentence_List)):
                    raise ValueError("style_token_weights must be [Head, Size], [1, Head, Size] or [batch, Head, Size]")
                style_embeddings = self.Style_Compose(tw)
            kwargs["style_embeddings"] = style_embeddings
        pattern_Dict = self.feeder.Get_Inference_Pattern(sentence_List, wav_List_for_GST, style_given=styled)
        if pattern_Dict is None:
            print("Inference fail.")
            return None
        if export:
            kwargs["with_vocoder"] = True
        out = self.Inference_Step(**pattern_Dict, **kwargs)
        self.synchronize()                     # the reference returns finished arrays; also where a give-up of this call surfaces
        if export:
            self.Export_Inference(sentence_List, out[0], out[1], out[2], out[3],
                                  label or datetime.now().strftime("%Y%m%d.%H%M%S"), vocoder=vocoder, seeds=seeds)
        return out

    # ------------------------------------------------------------------ the neural vocoder
    def _check_vocoder(self, vocoder):
        if vocoder not in ("griffin_lim", "melgan", "waveglow", "hifigan"):
            raise ValueError("vocoder must be 'griffin_lim', 'melgan', 'waveglow' or 'hifigan'")
        if vocoder == "melgan" and self._melgan is None:
            raise capi.GstTacoError(-4, "vocoder='melgan' needs Load_Neural_Vocoder first")
        if vocoder == "waveglow" and self._waveglow is None:
            raise capi.GstTacoError(-4, "vocoder='waveglow' needs Load_WaveGlow first")
        if vocoder == "hifigan" and self._hifigan is None:
            raise capi.GstTacoError(-4, "vocoder='hifigan' needs Load_HiFiGAN first")

    def _load_vocoder(self, module, section, prefix, weights_or_path, config, max_frames, hop_message, infer=None, operands=None, check=False):
        """What the three ``Load_*`` of the vocoders share: ``module`` is melgan / hifigan / waveglow, ``section`` its Hyper_Parameters
        section, ``prefix`` its name in capi.  ``infer``: the configuration of a set of arrays where ``module.infer_config(weights)``
        lacks an argument; ``operands``: HiFi-GAN's operand form, set between configure and the weights; ``check``: the configuration
        has size rules of its own to run first (``cfg.check()``: WaveGlow).  Returns the configuration."""
        if weights_or_path is None:
            weights_or_path = (self.hp_Dict.get(section) or {}).get("Checkpoint_Path")
            if weights_or_path is None:
                raise ValueError("no weights given and Hyper_Parameters has no {}.Checkpoint_Path".format(section))
        weights = module.load(weights_or_path) if isinstance(weights_or_path, (str, os.PathLike)) else weights_or_path
        cfg = config or module.from_hp(self.hp_Dict) or (infer or module.infer_config)(weights)
        if check:
            cfg.check()
        if cfg.mel_dim != self.dims.mel:
            raise ValueError("the vocoder's mel_dim {} is not Sound.Mel_Dim {}".format(cfg.mel_dim, self.dims.mel))
        if self.dims.audio and cfg.hop != self.dims.frame_shift:
            raise ValueError(hop_message.format(cfg.hop, self.dims.frame_shift))
        module.check_weights(cfg, weights)
        if not torch.cuda.is_available():
            raise capi.GstTacoError(-2, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)")
        getattr(self.ctx, prefix + "_configure")(cfg, self.ctx.cfg.max_batch, int(max_frames or self.dims.max_step))
        if operands is not None:
            self.ctx.hifigan_set_operands(operands)
        getattr(self.ctx, prefix + "_load_weights")(weights)
        with torch.cuda.device(self.device):
            getattr(self.ctx, prefix + "_finalize")()
        return cfg

    def _vocoder_io(self, cfg, mels, mel_lengths):
        """The mel check and the outputs of the three synthesis methods: (x, frames or None, B, T, ld, wav [B, ld], lengths [B])"""
        x = self._dev(mels, torch.float32)
        if x.dim() != 3 or x.shape[2] != cfg.mel_dim or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("mels must be [batch, frames >= 1, Mel_Dim]")
        B, T = int(x.shape[0]), int(x.shape[1])
        fr = self._dev(mel_lengths, torch.int32)
        if fr is not None and tuple(fr.shape) != (B,):
            raise ValueError("mel_lengths must be [batch]")
        ld = T * cfg.hop
        wav = torch.empty((B, ld), dtype=torch.float32, device=self.device)
        lens = torch.empty((B,), dtype=torch.int32, device=self.device)
        return x, fr, B, T, ld, wav, lens

    def Load_Neural_Vocoder(self, weights_or_path=None, config=None, max_frames=None):
        """Extension: loads the MelGAN generator (``gsttaco_melgan_*``, gst_tacotron_amd.melgan) into this model's context, once.
        ``weights_or_path``: named folded arrays (``melgan.synthetic_weights`` / ``melgan.from_state_dict``) or the path of a
        generator checkpoint in the public layout (``melgan.load``; None: ``Vocoder_MelGAN.Checkpoint_Path``).  ``config``: a ``melgan.MelGANConfig``; by default the
        Hyper_Parameters' ``Vocoder_MelGAN`` section, else what the arrays' shapes say.  ``max_frames``: the longest mel a call may
        bring (default Max_Step); the batch capacity is the model's.  Its Mel_Dim must be the model's and, where the Sound section
        is complete, its hop Sound.Frame_Shift."""
        from . import melgan
        self._melgan = self._load_vocoder(melgan, "Vocoder_MelGAN", "melgan", weights_or_path, config, max_frames,
                                          "the vocoder's ratios multiply to {}, Sound.Frame_Shift is {}")
        return self

    def Neural_Vocoder(self, mels, mel_lengths=None):
        """Extension: mels [B, T, Mel_Dim], normalised exactly as ``Inference_Step`` and ``Inference_GTA`` produce them (what a vocoder
        trained on GTA mels sees: no de-normalisation), torch or numpy, with ``mel_lengths`` [B] or None (all frames) ->
        (wav float32 [B, T * hop] in [-1, 1], wav_lengths int32 [B]) on the device (``gsttaco_melgan``).  Row b uses its own
        ``mel_lengths[b]`` frames everywhere -- its samples are bitwise those of the row run alone -- and is zero beyond
        ``wav_lengths[b] = mel_lengths[b] * hop``; rows shorter than the vocoder's ``min_frames`` come out with length 0."""
        if self._melgan is None:
            raise capi.GstTacoError(-4, "no neural vocoder loaded (call Load_Neural_Vocoder first)")
        x, fr, B, T, ld, wav, lens = self._vocoder_io(self._melgan, mels, mel_lengths)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_melgan(self.ctx.handle, _ptr(x), _ptr(fr), B, T, _ptr(wav), _ptr(lens), ld, self._stream()))
        return wav, lens

    # ------------------------------------------------------------------ the flow vocoder
    def Load_HiFiGAN(self, weights_or_path=None, config=None, max_frames=None, precision=None):
        """Extension: loads the HiFi-GAN generator (``gsttaco_hifigan_*``, gst_tacotron_amd.hifigan) into this model's context, once,
        beside or without the MelGAN generator and WaveGlow.  ``weights_or_path``: named folded arrays (``hifigan.synthetic_weights``
        / ``hifigan.from_state_dict``) or the path of a file that holds a generator ``state_dict`` in the public layout
        (``hifigan.load``; None: ``Vocoder_HiFiGAN.Checkpoint_Path``).  ``config``: a ``hifigan.HiFiGANConfig``; by default the
        Hyper_Parameters' ``Vocoder_HiFiGAN`` section, else what the arrays' shapes say (the dilations only for the shipped shapes).
        ``max_frames``: the longest mel a call may bring (default Max_Step); the batch capacity is the model's.  Its Mel_Dim must be
        the model's and, where the Sound section is complete, its hop Sound.Frame_Shift.
        ``precision``: the operand type of the generator's matrix products, "float32" (the default), "bfloat16" or "float16"
        (``gsttaco_hifigan_set_operands``: 16-bit MFMA operands, everything else fp32; None: ``Vocoder_HiFiGAN.Precision``, else
        "float32").  ``Use_Mixed_Precision`` does not switch it.  ``HiFiGAN``, ``Inference(..., vocoder="hifigan")`` and
        ``Export_Inference`` use whatever was loaded; their outputs are float32 in [-1, 1] in every form."""
        from . import hifigan
        precision = hifigan.precision_from_hp(self.hp_Dict) if precision is None else hifigan.check_precision(precision)
        self._hifigan = self._load_vocoder(hifigan, "Vocoder_HiFiGAN", "hifigan", weights_or_path, config, max_frames,
                                           "the vocoder's rates multiply to {}, Sound.Frame_Shift is {}",
                                           operands=None if precision == "float32" else precision)
        self._hifigan_precision = precision
        return self

    def HiFiGAN(self, mels, mel_lengths=None):
        """Extension: mels [B, T, Mel_Dim], normalised exactly as ``Inference_Step`` and ``Inference_GTA`` produce them (what a vocoder
        trained on GTA mels sees: no de-normalisation), torch or numpy, with ``mel_lengths`` [B] or None (all frames) ->
        (wav float32 [B, T * hop] in [-1, 1], wav_lengths int32 [B]) on the device (``gsttaco_hifigan``).  Row b uses its own
        ``mel_lengths[b]`` frames everywhere -- its samples are bitwise those of the row run alone -- and is zero beyond
        ``wav_lengths[b] = mel_lengths[b] * hop``; one frame is enough, a row of 0 frames comes out with length 0."""
        if self._hifigan is None:
            raise capi.GstTacoError(-4, "no HiFi-GAN loaded (call Load_HiFiGAN first)")
        x, fr, B, T, ld, wav, lens = self._vocoder_io(self._hifigan, mels, mel_lengths)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_hifigan(self.ctx.handle, _ptr(x), _ptr(fr), B, T, _ptr(wav), _ptr(lens), ld, self._stream()))
        return wav, lens

    def Load_WaveGlow(self, weights_or_path=None, config=None, max_frames=None):
        """Extension: loads WaveGlow (``gsttaco_waveglow_*``, gst_tacotron_amd.waveglow) into this model's context, once, beside or
        without the MelGAN generator.  ``weights_or_path``: named folded arrays (``waveglow.synthetic_weights`` /
        ``waveglow.from_state_dict``) or the path of a file that holds a ``state_dict`` in the public layout (``waveglow.load``; None:
        ``Vocoder_WaveGlow.Checkpoint_Path``).  ``config``: a ``waveglow.WaveGlowConfig``; by default the Hyper_Parameters'
        ``Vocoder_WaveGlow`` section, else what the arrays' shapes say at hop = Sound.Frame_Shift.  ``max_frames``: the longest mel a
        call may bring (default Max_Step); the batch capacity is the model's.  Its Mel_Dim must be the model's and, where the Sound
        section is complete, its hop Sound.Frame_Shift."""
        from . import waveglow
        self._waveglow = self._load_vocoder(waveglow, "Vocoder_WaveGlow", "waveglow", weights_or_path, config, max_frames,
                                            "the vocoder's hop {} is not Sound.Frame_Shift {}",
                                            infer=lambda w: waveglow.infer_config(w, hop=int(self.hp_Dict["Sound"]["Frame_Shift"])), check=True)
        return self

    def WaveGlow(self, mels, mel_lengths=None, sigma=0.6, seeds=None, z=None):
        """Extension: mels [B, T, Mel_Dim], normalised exactly as ``Inference_Step`` and ``Inference_GTA`` produce them, torch or numpy,
        with ``mel_lengths`` [B] or None (all frames) -> (wav float32 [B, T * hop], wav_lengths int32 [B]) on the device
        (``gsttaco_waveglow``).  The waveform is sampled: ``sigma`` is the temperature, and the noise is either drawn on the device from
        ``seeds`` [B] (integers mod 2^64; None: 0 for every row) or given as ``z`` [B, T * hop] -- not both.  A row's noise depends on its
        seed and the sample's position only, and row b uses its own ``mel_lengths[b]`` frames everywhere: its samples are bitwise those
        of the row run alone.  The output is NOT bounded by 1 (a flow has no tanh); the WAV writer clips.  Beyond
        ``wav_lengths[b] = mel_lengths[b] * hop`` a row is zeros."""
        if self._waveglow is None:
            raise capi.GstTacoError(-4, "no flow vocoder loaded (call Load_WaveGlow first)")
        if seeds is not None and z is not None:
            raise ValueError("seeds and z are mutually exclusive")
        x, fr, B, T, ld, wav, lens = self._vocoder_io(self._waveglow, mels, mel_lengths)
        dev_seeds = None
        if z is not None:
            z = self._dev(z, torch.float32)
            if tuple(z.shape) != (B, ld):
                raise ValueError("z must be [batch, frames * hop]")
        else:
            if seeds is None:
                seeds = [0] * B
            if torch.is_tensor(seeds):
                seeds = seeds.cpu().numpy()
            vals = [int(v) & checked.MASK64 for v in np.asarray(seeds, dtype=object).reshape(-1)]
            if np.ndim(seeds) != 1 or len(vals) != B:
                raise ValueError("seeds must be [batch]")
            dev_seeds = torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64)).to(self.device)      # (the same 64 bits)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_waveglow(self.ctx.handle, _ptr(x), _ptr(fr), B, T, ctypes.c_float(float(sigma)),
                                                         _ptr(dev_seeds), _ptr(z), _ptr(wav), _ptr(lens), ld, self._stream()))
        return wav, lens

    def Inference_Checked(self, sentence_List, wav_List_for_GST=None, style_embeddings=None, style_token_weights=None, seeds=None,
                          max_attempts=3, accept=None, export=False, label=None, **kwargs):
        """Extension: ``Inference`` that reads the synthesis report of what it made and redoes only the utterances that failed.
        Attempt k (0 = the first) of utterance i runs under seed ``(seeds[i] + k * 0x9E3779B97F4A7C15) mod 2^64`` (``seeds`` defaults to
        consecutive values from the model's counter), masked and with per-utterance seeds, so every returned utterance is the one
        ``Inference_Step`` gives for that sentence, style and seed ALONE.  After each attempt ``Utterance_Report`` runs and
        ``accept(report_row, focus, i, k)`` decides; the default accepts when the stop token fired (``stop_step < S``), the attention
        reached the last token (``end_gap == 0``) and nothing is non-finite -- no thresholds.  Rejected utterances run again as a
        smaller batch of their own and replace their outputs, until all are accepted or ``max_attempts`` attempts are made (the last
        attempt's outputs stay; the default ``accept`` on the returned report tells).
        Returns (mels: list of [frames_i, Mel_Dim] trimmed to the report's ``frames``, report int32 [B, 8], focus [B], attempts int32
        [B] -- the attempt each row comes from --, stops [B, S], alignments [B, S, T_v] untrimmed; alignments of a re-run batch are
        zero-padded to the first attempt's T_v).  ``export=True``: the final mels go through the vocoder, ``Inv_Spectrogram`` takes
        ``frames`` from the report on the device and the wavs are written where ``Export_Inference`` writes them; their paths are
        appended to the returned tuple.
        The shrinking batches are new shapes to the graph cache: each is captured at its first use by default.  Callers that run
        this repeatedly should ``set_graph_policy(capture_after=2)`` so that only batch sizes that come back are captured."""
        print("Checked inference running...")
        n = len(sentence_List)
        for k in ("seed", "prenet_masks", "attn_noise", "masked", "with_vocoder", "return_pre_mel", "teacher_mels"):
            if k in kwargs:
                raise ValueError("Inference_Checked sets '{}' itself".format(k))
        styled = style_embeddings is not None or style_token_weights is not None
        if styled:
            if wav_List_for_GST is not None or (style_embeddings is not None and style_token_weights is not None):
                raise ValueError("wav_List_for_GST, style_embeddings and style_token_weights are mutually exclusive")
            if not self.hp_Dict["GST"]["Use"]:
                raise ValueError("GST is not used")
            if style_token_weights is not None:
                tw = self._dev(style_token_weights, torch.float32)
                style_embeddings = self.Style_Compose(tw.unsqueeze(0) if tw.dim() == 2 else tw)
            style_embeddings = self._dev(style_embeddings, torch.float32)
            if style_embeddings.dim() != 2 or style_embeddings.shape[0] not in (1, n):
                raise ValueError("style_embeddings must be [batch, A] or [1, A]")
        pattern = self.feeder.Get_Inference_Pattern(sentence_List, wav_List_for_GST, style_given=styled)
        if pattern is None:
            print("Inference fail.")
            return None
        pattern.pop("initial_mels", None)
        if styled:
            pattern["style_embeddings"] = style_embeddings
        if seeds is None:
            seeds = [self.seed + 1 + i for i in range(n)]
            self.seed += n
        seeds = [int(v) for v in (seeds.tolist() if hasattr(seeds, "tolist") else seeds)]
        if len(seeds) != n:
            raise ValueError("seeds must hold one seed per sentence")
        lengths = np.asarray(pattern["token_lengths"])
        final = {}

        def take(a, rows):
            if a.shape[0] != n:                 # (one style for the whole batch)
                return a
            return a[torch.as_tensor(rows, device=a.device)] if torch.is_tensor(a) else a[np.asarray(rows)]

        def run(rows, row_seeds):
            sub = {k: take(v, rows) for k, v in pattern.items()}
            sub["tokens"] = np.ascontiguousarray(sub["tokens"][:, :int(lengths[rows].max())])
            mel, stop, _, align = self.Inference_Step(**sub, seeds=row_seeds, masked=True, **kwargs)
            report, focus = self.Utterance_Report(stop, align, sub["token_lengths"], mel)
            if not final:                       # (attempt 0 is every row: its outputs, in copies of their own, are the store)
                final.update(mel=mel.clone(), stop=stop.clone(), align=align.clone(), report=report.clone(), focus=focus.clone())
            else:
                at = torch.as_tensor(rows, device=self.device)
                for key, v in (("mel", mel), ("stop", stop), ("report", report), ("focus", focus)):
                    final[key][at] = v
                final["align"][at] = 0.0
                final["align"][at, :, :align.shape[2]] = align
            self.synchronize()                  # (where a give-up of this attempt surfaces; the report is read on the host next)
            return report.cpu().numpy(), focus.cpu().numpy()

        S = self.dims.steps if kwargs.get("steps") is None else int(kwargs["steps"])
        attempts, _ = checked.run_checked(seeds, max_attempts, run, accept or checked.default_accept(S))
        frames = final["report"][:, 1].cpu().numpy()
        out = ([final["mel"][i, :int(frames[i])] for i in range(n)], final["report"], final["focus"],
               torch.as_tensor(attempts, dtype=torch.int32), final["stop"], final["align"])
        if export:
            from . import export as export_mod
            spec = self.vocoder(final["mel"])
            wav, lens = self.Inv_Spectrogram(spec, frames=final["report"][:, 1].contiguous())
            wav, lens = wav.cpu().numpy(), lens.cpu().numpy()
            root = self.hp_Dict["Inference_Path"]
            os.makedirs(os.path.join(root, "Wav"), exist_ok=True)
            label = label or datetime.now().strftime("%Y%m%d.%H%M%S")
            paths = []
            for i in range(n):
                paths.append(os.path.join(root, "Wav", "{}.IDX_{}.WAV".format(label, i)))
                export_mod.write_wav(paths[-1], wav[i, :lens[i]], self.dims.sample_rate)
            out = out + (paths,)
        return out

    def Inv_Spectrogram(self, spectrograms, frames=None, iters=None, power=1.5, ref_level_db=20.0, init_phase=None, seed=0):
        """Batched reference Audio.inv_spectrogram (Audio.py:23-27) on the GPU: spectrograms [B, T, Spectrogram_Dim] as
        Inference_Step returns them -> (wav [B, Frame_Shift*(T-1)] float32, wav_lengths [B]).  ``frames`` [B] limits the
        frames used per utterance; ``init_phase`` [B,T,Spectrogram_Dim] in [0,1) injects the random initial phases."""
        d = self.dims
        if not d.audio or not self.ctx.cfg.max_wav_samples:
            raise ValueError("the audio back end needs the Sound section of Hyper_Parameters and max_wav_seconds > 0")
        if not torch.cuda.is_available():
            raise capi.GstTacoError(-2, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)")
        spec = self._dev(spectrograms, torch.float32)
        B, T = spec.shape[0], spec.shape[1]
        if iters is None:
            iters = int(self.hp_Dict.get("Vocoder_Taco1", {}).get("Griffin-Lim_Iter", 60))
        fr = self._dev(frames, torch.int32)
        ph = self._dev(init_phase, torch.float32)
        ld = max(1, d.frame_shift * (T - 1))
        wav = torch.empty((B, ld), dtype=torch.float32, device=self.device)
        lens = torch.empty((B,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_griffin_lim(
                self.ctx.handle, _ptr(spec), _ptr(fr), B, T, int(iters), ctypes.c_float(float(power)),
                ctypes.c_float(float(ref_level_db)), _ptr(ph), ctypes.c_uint64(int(seed)), _ptr(wav), _ptr(lens), ld,
                self._stream()))
        return wav, lens

    def Export_Inference(self, sentence_List, mel_List, stop_List, spectrogram_List, alignment_List, label, plot=True, vocoder="griffin_lim",
                         seeds=None):
        """reference Model.py:369-427: per utterance a figure (Plot/<label>.IDX_<i>.PNG) and the Griffin-Lim wav of the
        spectrogram cut at the stop token (Wav/<label>.IDX_<i>.WAV) under Inference_Path.  Returns the wav paths.
        ``vocoder="melgan"`` (extension): the WAVs are ``Neural_Vocoder`` of the post-net mels, cut at the ``frames`` column of
        ``Utterance_Report``, in place of Griffin-Lim; the figures are unchanged.  ``vocoder="waveglow"``: ``WaveGlow`` of the same cut
        mels at its default temperature, row b's noise drawn from ``seeds[b]`` (None: 0 for every row).  ``vocoder="hifigan"``:
        ``HiFiGAN`` of the same cut mels."""
        from . import export
        self._check_vocoder(vocoder)
        root = self.hp_Dict["Inference_Path"]
        os.makedirs(os.path.join(root, "Plot"), exist_ok=True)
        os.makedirs(os.path.join(root, "Wav"), exist_ok=True)
        stops = np.asarray(stop_List.cpu() if torch.is_tensor(stop_List) else stop_List, dtype=np.float32)
        slice_idx = [export.stop_slice_index(s) for s in stops]
        frames = np.array([max(1, i) * self.dims.r for i in slice_idx], dtype=np.int32)           # Model.py:415
        if vocoder == "melgan":
            report, _ = self.Utterance_Report(stop_List, alignment_List)
            wav, lens = self.Neural_Vocoder(mel_List, report[:, 1].contiguous())
        elif vocoder == "waveglow":
            report, _ = self.Utterance_Report(stop_List, alignment_List)
            wav, lens = self.WaveGlow(mel_List, report[:, 1].contiguous(), seeds=seeds)
        elif vocoder == "hifigan":
            report, _ = self.Utterance_Report(stop_List, alignment_List)
            wav, lens = self.HiFiGAN(mel_List, report[:, 1].contiguous())
        else:
            wav, lens = self.Inv_Spectrogram(spectrogram_List, frames=frames)
        wav, lens = wav.cpu().numpy(), lens.cpu().numpy()
        to_np = lambda a: np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.float32)
        mels, specs, aligns = to_np(mel_List), to_np(spectrogram_List), to_np(alignment_List)
        paths = []
        for i, sentence in enumerate(sentence_List):
            if plot:
                try:
                    export.plot_inference(os.path.join(root, "Plot", "{}.IDX_{}.PNG".format(label, i)), sentence, mels[i],
                                          specs[i], aligns[i], stops[i], slice_idx[i])
                except ImportError:
                    plot = False                      # matplotlib is optional
            p = os.path.join(root, "Wav", "{}.IDX_{}.WAV".format(label, i))
            export.write_wav(p, wav[i, :lens[i]], self.dims.sample_rate)
            paths.append(p)
        return paths

    def Export_GST(self, wav_List, tag_List, gst_List, label):
        """reference Model.py:448-459"""
        from . import export
        gst = np.asarray(gst_List.cpu() if torch.is_tensor(gst_List) else gst_List)
        path = os.path.join(self.hp_Dict["Inference_Path"], "GST", "{}.GST.TXT".format(label))
        export.export_gst(path, wav_List, tag_List, gst)
        return path

    def Export_GST_Map(self, wav_List, tag_List, y, label):
        """The style map of ``Inference_GST(..., style_map=...)`` as GST/<label>.GST.MAP.TXT and, where matplotlib imports,
        GST/<label>.GST.PNG (what reference R_Script/TSNE.R saves).  Returns the table's path."""
        from . import export
        y = np.asarray(y.cpu() if torch.is_tensor(y) else y, dtype=np.float64)
        root = os.path.join(self.hp_Dict["Inference_Path"], "GST")
        path = os.path.join(root, "{}.GST.MAP.TXT".format(label))
        export.export_gst_map(path, wav_List, tag_List, y)
        try:
            export.plot_gst_map(os.path.join(root, "{}.GST.PNG".format(label)), tag_List, y)
        except ImportError:
            pass                                  # matplotlib is optional
        return path

    # ------------------------------------------------------------------ per-phase entry points (tests / profiling)
    def decode_plan(self, Tv):
        """(fused_front, fused_prenet0, lean) -- which variant of the decode step a Tv-token batch runs on
        (``gsttaco_decode_plan``).  The mixed-precision parity oracle needs ``fused_prenet0``."""
        self._require_ready()
        plan = (ctypes.c_int32 * 3)()
        self.ctx.check(self.ctx.lib.gsttaco_decode_plan(self.ctx.handle, int(Tv), plan))
        return bool(plan[0]), bool(plan[1]), bool(plan[2])

    def decode_plan_fields(self, B, Tv, forced=False):
        """{field: int} -- the whole launch plan of one decode of ``B`` utterances of ``Tv`` tokens (``forced``: teacher-forced), as
        the function that enqueues it decides it: ``capi.PLAN_FIELDS`` (``gsttaco_decode_plan_fields``; test support)."""
        self._require_ready()
        out = (ctypes.c_int32 * len(capi.PLAN_FIELDS))()
        self.ctx.check(self.ctx.lib.gsttaco_decode_plan_fields(self.ctx.handle, int(B), int(Tv), int(bool(forced)), out))
        return dict(zip(capi.PLAN_FIELDS, (int(v) for v in out)))

    def set_graph_policy(self, max_cached=8, capture_after=1):
        """hipGraph cache policy (``gsttaco_set_graph_policy``): at most ``max_cached`` graph executables are kept (LRU);
        a shape is captured at its ``capture_after``-th use and enqueued eagerly before.  Use ``capture_after=2`` when
        batch shapes vary from call to call (the reference's Feeder pads to the batch maximum, Feeder.py:175-180)."""
        self.ctx.check(self.ctx.lib.gsttaco_set_graph_policy(self.ctx.handle, int(max_cached), int(capture_after)))

    def synchronize(self):
        """Synchronises the current stream and raises GstTacoError if a hand-off wait of the persistent decode launch, of a persistent
        BiLSTM launch or of a fused decode-LSTM launch gave up since the last check (``gsttaco_synchronize``, the one place that clears the condition): the
        outputs of the calls since then are invalid and should be repeated -- the context runs the launch-per-step forms from
        then on.  ``Inference`` calls this before it returns."""
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_synchronize(self.ctx.handle, self._stream()))

    def last_message(self):
        """The library's last error or warning text for this context (``gsttaco_last_error``)."""
        return self.ctx.lib.gsttaco_last_error(self.ctx.handle).decode()

    def handoff_error(self):
        """Non-zero while a give-up is pending on this context, i.e. raised and not yet reported by ``synchronize`` (bit 0: fused
        decode-LSTM launch, bit 8: persistent BiLSTM, bit 16: persistent decode launch; ``gsttaco_debug_handoff_error``)."""
        out = ctypes.c_uint32(0)
        self.ctx.check(self.ctx.lib.gsttaco_debug_handoff_error(self.ctx.handle, ctypes.byref(out)))
        return int(out.value)

    def debug_counters(self):
        """(persistent BiLSTM launches this context has enqueued, 1 while the context still uses the persistent launch) --
        ``gsttaco_debug_counters``."""
        out = (ctypes.c_uint64 * 4)()
        self.ctx.check(self.ctx.lib.gsttaco_debug_counters(self.ctx.handle, out))
        return int(out[0]), int(out[1])

    def decode_counters(self):
        """(persistent decode launches this context has enqueued, 1 while the context still uses the persistent decode launch) --
        the whole decoder loop as ONE launch (``csrc/persist_decode.hip``; ``gsttaco_debug_counters`` out[2:4])."""
        out = (ctypes.c_uint64 * 4)()
        self.ctx.check(self.ctx.lib.gsttaco_debug_counters(self.ctx.handle, out))
        return int(out[2]), int(out[3])

    def graph_cache_size(self):
        return int(self.ctx.lib.gsttaco_graph_cache_size(self.ctx.handle))

    def debug_randomness(self, steps, B, Tv):
        """(prenet_masks [steps, 2, B, P], attn_noise [steps, B, Tv]) the last decode of that shape used, as NumPy arrays in
        the layout ``Inference_Step(prenet_masks=, attn_noise=)`` takes -- in throughput mode the tensors generated from the
        seed (``gsttaco_debug_randomness``; test support)."""
        import numpy as np
        self._require_ready()
        d = self.dims
        P0, P1 = d.prenet[0], d.prenet[1]
        if P0 != P1:
            raise ValueError("debug_randomness returns a stacked mask tensor: equal prenet sizes only")
        masks = np.empty((steps, B * (P0 + P1)), np.float32)
        noise = np.empty((steps, B, Tv), np.float32)
        self.ctx.check(self.ctx.lib.gsttaco_debug_randomness(self.ctx.handle, masks.ctypes.data_as(ctypes.c_void_p),
                                                             noise.ctypes.data_as(ctypes.c_void_p), int(steps), int(B), int(Tv)))
        return masks.reshape(steps, 2, B, P0), noise

    def encode(self, tokens, token_lengths=None):
        self._require_ready()
        tok = self._dev(tokens, torch.int32)
        tlen = self._dev(token_lengths, torch.int32)
        B, Tv = tok.shape
        enc = torch.empty((B, Tv, self.dims.enc_out), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_encode(self.ctx.handle, _ptr(tok), _ptr(tlen), B, Tv, _ptr(enc), self._stream()))
        return enc

    def decode(self, enc, gst=None, prenet_masks=None, attn_noise=None, seed=0, steps=None, token_lengths=None, teacher_mels=None,
               seeds=None):
        """``gsttaco_decode``; with ``teacher_mels`` [B, Tq, Mel_Dim] (see ``Inference_Step``) ``gsttaco_decode_forced``.  ``seeds`` [B]:
        per-utterance seeds (see ``Inference_Step``) in place of ``seed`` (left at 0), ``prenet_masks`` and ``attn_noise``."""
        self._require_ready()
        d = self.dims
        enc = self._dev(enc, torch.float32)
        gst = self._dev(gst, torch.float32)
        tlen = self._dev(token_lengths, torch.int32)
        B, Tv = enc.shape[0], enc.shape[1]
        teacher, Tq = self._teacher(teacher_mels, B, steps)
        S = (Tq - 1 + d.r - 1) // d.r if teacher is not None else d.steps if steps is None else int(steps)
        if seeds is not None:
            self._seeds_exclusive(seed or None, prenet_masks, attn_noise)
            prenet_masks, attn_noise = self.Fill_Randomness(seeds, S, Tv, batch=B)
        masks = self._dev(prenet_masks, torch.float32)
        noise = self._dev(attn_noise, torch.float32)
        pre = torch.empty((B, S * d.r, d.mel), dtype=torch.float32, device=self.device)
        stop = torch.empty((B, S), dtype=torch.float32, device=self.device)
        align = torch.empty((B, S, Tv), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            if teacher is not None:
                self.ctx.check(self.ctx.lib.gsttaco_decode_forced(
                    self.ctx.handle, _ptr(enc), _ptr(gst), _ptr(tlen), _ptr(masks), _ptr(noise), ctypes.c_uint64(int(seed)),
                    B, Tv, _ptr(teacher), Tq, _ptr(pre), _ptr(stop), _ptr(align), self._stream()))
                return pre, stop, align
            self.ctx.check(self.ctx.lib.gsttaco_decode(
                self.ctx.handle, _ptr(enc), _ptr(gst), _ptr(tlen), _ptr(masks), _ptr(noise), ctypes.c_uint64(int(seed)),
                B, Tv, S, _ptr(pre), _ptr(stop), _ptr(align), self._stream()))
        return pre, stop, align

    def vocoder(self, mel):
        """Vocoder_Taco1 alone: mel [B,T,Mel_Dim] -> linear spectrogram [B,T,Spectrogram_Dim] (reference Taco2.py:234-260)."""
        self._require_ready()
        x = self._dev(mel, torch.float32)
        B, T = x.shape[0], x.shape[1]
        spec = torch.empty((B, T, self.dims.spec), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_vocoder(self.ctx.handle, _ptr(x), B, T, _ptr(spec), self._stream()))
        return spec

    def postnet_variants(self, B, T):
        """The conv/GEMM dispatcher variant (capi.CONV_V / capi.CONV_VH ids) each postnet layer runs at (B, T)."""
        self._require_ready()
        v = (ctypes.c_int32 * 8)()
        self.ctx.check(self.ctx.lib.gsttaco_postnet_variants(self.ctx.handle, B, T, v))
        return [int(v[i]) for i in range(min(len(self.dims.post_filters), 8))]

    def encoder_variants(self, B, Tv):
        """(the dispatcher variant each encoder conv layer runs at (B, Tv), whether the embedding lookup is launched as rows in front
        of layer 0) -- ``gsttaco_encoder_variants``."""
        self._require_ready()
        v, rows = (ctypes.c_int32 * 8)(), ctypes.c_int32(0)
        self.ctx.check(self.ctx.lib.gsttaco_encoder_variants(self.ctx.handle, B, Tv, v, ctypes.byref(rows)))
        return [int(v[i]) for i in range(min(len(self.dims.enc_filters), 8))], bool(rows.value)

    def vocoder_variants(self, B, T):
        """{kind: [dispatcher variant of each of the vocoder's GEMMs of that kind at (B, T)]} over ``capi.VOC_KINDS``, in the order
        they are enqueued; a Dense the model does not have gives [] (``gsttaco_vocoder_variants``)."""
        self._require_ready()
        out = {}
        for kind, code in capi.VOC_KINDS.items():
            v, n = (ctypes.c_int32 * 32)(), ctypes.c_int32(0)
            self.ctx.check(self.ctx.lib.gsttaco_vocoder_variants(self.ctx.handle, code, B, T, v, ctypes.byref(n)))
            out[kind] = [int(v[i]) for i in range(min(int(n.value), 32))]
        return out

    def postnet(self, pre_mel):
        self._require_ready()
        pre = self._dev(pre_mel, torch.float32)
        B, T = pre.shape[0], pre.shape[1]
        mel = torch.empty_like(pre)
        with torch.cuda.device(self.device):
            self.ctx.check(self.ctx.lib.gsttaco_postnet(self.ctx.handle, _ptr(pre), B, T, _ptr(mel), self._stream()))
        return mel
