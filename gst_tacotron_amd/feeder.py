"""Inference-side input conventions of the reference Feeder (reference Feeder.py:161-252).

Only what the hot path's caller needs: tokenise / pad, zero ``initial_mels``, and the
``mels_for_gst`` batch layout (a zero frame is prepended, lengths exclude it).  Reference audio is given
like in the reference as wav paths (or 1-D sample arrays): the wav -> mel front end
(Pattern_Generator.Mel_Generate) then runs on the GPU through the ``mel_frontend`` callable the
model installs, and ``mels_for_gst`` comes back as a device tensor.  Precomputed mel arrays ``[T, Mel_Dim]``
in [-Max_Abs_Mel, Max_Abs_Mel] are accepted too (no GPU involved).
"""
import numpy as np

from .hparams import load_token_dict


class Feeder:
    def __init__(self, hp, token_index_dict=None, mel_frontend=None):
        self.hp = hp
        self.token_Index_Dict = token_index_dict or load_token_dict(hp)
        self.mel_frontend = mel_frontend          # callable(wav_List, top_db) -> (mels_for_gst, mel_lengths_for_gst)

    @staticmethod
    def _is_mel(item):
        # (a tuple is a (samples, rate) pair: audio at another rate, for the front end like a path)
        return not isinstance(item, (str, bytes, tuple)) and not hasattr(item, "__fspath__") and np.ndim(item) == 2

    def _from_wavs(self, wav_List, top_db):
        if self.mel_frontend is None:
            raise RuntimeError("wav inputs need the GPU mel front end (GST_Tacotron installs it); there is no CPU path")
        mels, lens = self.mel_frontend(wav_List, top_db)
        return {"mels_for_gst": mels, "mel_lengths_for_gst": lens}

    def Get_Inference_Pattern(self, sentence_List, mel_List_for_GST=None, style_given=False):
        """reference Feeder.py:161-227.  Out-of-vocabulary characters raise KeyError like the
        reference (Feeder.py:169); bad GST inputs print the reference's message and return None.
        ``style_given=True`` (extension): the caller supplies the style embedding itself
        (``Inference_Step(style_embeddings=...)``), so the token pattern is returned without the GST keys and no
        reference audio is asked for."""
        pattern_Count = len(sentence_List)
        sentence_List = [sentence.upper().strip() for sentence in sentence_List]          # :164
        token_List = [
            np.array([self.token_Index_Dict["<S>"]] + [self.token_Index_Dict[ch] for ch in s]
                     + [self.token_Index_Dict["<E>"]], dtype=np.int32)                     # :166-174
            for s in sentence_List]
        max_len = max(t.shape[0] for t in token_List)
        tokens = np.full((pattern_Count, max_len), self.token_Index_Dict["<E>"], dtype=np.int32)   # :177-180
        for i, t in enumerate(token_List):
            tokens[i, :t.shape[0]] = t
        mel_dim = self.hp["Sound"]["Mel_Dim"]
        pattern = {
            "tokens": tokens,
            "token_lengths": np.array([t.shape[0] for t in token_List], dtype=np.int32),
            "initial_mels": np.zeros((pattern_Count, 1, mel_dim), dtype=np.float32),        # :182-185
        }
        if self.hp["GST"]["Use"] and not style_given:
            if mel_List_for_GST is None:
                print("GST is enabled, but no wav information.")                           # :197-199
                return None
            if len(mel_List_for_GST) not in (1, pattern_Count):
                print("The length of wav_List_for_GST must be 1 or same to the length of sentence_List "
                      "and wav_List_for_GST must be same.")                                 # :200-202
                return None
            items = list(mel_List_for_GST)
            if all(self._is_mel(m) for m in items):
                pattern.update(self.Get_Inference_GST_Pattern(items * (pattern_Count if len(items) == 1 else 1)))
            elif len(items) == 1:
                # one reference wav for every sentence: top_db 60, the mel is repeated (Feeder.py:204-207)
                one = self._from_wavs(items, 60)
                pattern["mels_for_gst"] = one["mels_for_gst"].expand(pattern_Count, -1, -1).contiguous()
                pattern["mel_lengths_for_gst"] = one["mel_lengths_for_gst"].expand(pattern_Count).contiguous()
            else:
                pattern.update(self._from_wavs(items, 15))        # several wavs: top_db 15 (Feeder.py:209)
        return pattern

    def Get_Inference_GST_Pattern(self, mel_List):
        """reference Feeder.py:229-252: zero-pad to the longest mel, PREPEND one zero frame.  Wav paths / sample
        arrays go through the GPU front end with top_db 60 (Feeder.py:232)."""
        mel_dim = self.hp["Sound"]["Mel_Dim"]
        if not all(self._is_mel(m) for m in mel_List):
            return self._from_wavs(list(mel_List), 60)
        mel_List = [np.asarray(m, dtype=np.float32) for m in mel_List]
        for m in mel_List:
            if m.ndim != 2 or m.shape[1] != mel_dim or m.shape[0] < 1:
                raise ValueError("reference mels must be [T>=1, {}] arrays".format(mel_dim))
        max_len = max(m.shape[0] for m in mel_List)
        mels = np.zeros((len(mel_List), max_len + 1, mel_dim), dtype=np.float32)
        for i, m in enumerate(mel_List):
            mels[i, 1:m.shape[0] + 1] = m
        return {"mels_for_gst": mels,
                "mel_lengths_for_gst": np.array([m.shape[0] for m in mel_List], dtype=np.int32)}

    def Get_Teacher_Pattern(self, sentence_List, mel_List):
        """Extension (teacher forcing, ``GST_Tacotron.Inference_Step(teacher_mels=...)``): tokens as ``Get_Inference_Pattern`` makes them
        and the target mels [T, Mel_Dim] in the layout the reference trains on (Feeder.py:103-143): zero-padded to the longest, a zero
        go frame PREPENDED, padded to a multiple of Step_Reduction, and one more frame appended (the decoder reads ``mels[:, 0:-1:r]``,
        Taco2.py:161).  Returns tokens, token_lengths, teacher_mels [B, Tq, Mel_Dim] and mel_lengths [B] (excluding the go frame)."""
        if len(mel_List) != len(sentence_List):
            raise ValueError("mel_List must hold one mel per sentence")
        mel_dim, r = self.hp["Sound"]["Mel_Dim"], int(self.hp["Step_Reduction"])
        mel_List = [np.asarray(m, dtype=np.float32) for m in mel_List]
        for m in mel_List:
            if m.ndim != 2 or m.shape[1] != mel_dim or m.shape[0] < 1:
                raise ValueError("teacher mels must be [T>=1, {}] arrays".format(mel_dim))
        pattern = self.Get_Inference_Pattern(sentence_List, style_given=True)
        del pattern["initial_mels"]
        max_len = max(m.shape[0] for m in mel_List)
        padded = -(-(max_len + 1) // r) * r                         # Feeder.py:132-133 (go frame included)
        mels = np.zeros((len(mel_List), padded + 1, mel_dim), dtype=np.float32)      # :134-137 (+1: dropped by 0:-1:r)
        for i, m in enumerate(mel_List):
            mels[i, 1:m.shape[0] + 1] = m
        pattern["teacher_mels"] = mels
        pattern["mel_lengths"] = np.array([m.shape[0] for m in mel_List], dtype=np.int32)
        return pattern

    def Get_Evaluation_Pattern(self, sentence_List, mel_List, spectrogram_List=None):
        """Extension (``GST_Tacotron.Evaluate``): ``Get_Teacher_Pattern`` plus the linear spectrogram targets [T, Spectrogram_Dim] in the
        layout the reference's training batch has (Feeder.py:103-143): both padded to ONE length -- the longer of the two, go frame
        included, rounded up to Step_Reduction (:134-135) -- plus the frame that ``mels[:, 0:-1:r]`` drops.  Adds ``spectrograms``
        [B, Tq, Spectrogram_Dim] and ``spectrogram_lengths`` [B]; without ``spectrogram_List`` it is ``Get_Teacher_Pattern``."""
        pattern = self.Get_Teacher_Pattern(sentence_List, mel_List)
        if spectrogram_List is None:
            return pattern
        if len(spectrogram_List) != len(sentence_List):
            raise ValueError("spectrogram_List must hold one spectrogram per sentence")
        spec_dim, r = int(self.hp["Sound"]["Spectrogram_Dim"]), int(self.hp["Step_Reduction"])
        spec_List = [np.asarray(s, dtype=np.float32) for s in spectrogram_List]
        for s in spec_List:
            if s.ndim != 2 or s.shape[1] != spec_dim or s.shape[0] < 1:
                raise ValueError("spectrogram targets must be [T>=1, {}] arrays".format(spec_dim))
        mels = pattern["teacher_mels"]
        longest = max(int(pattern["mel_lengths"].max()), max(s.shape[0] for s in spec_List))
        padded = -(-(longest + 1) // r) * r                         # Feeder.py:134-135 (go frame included)
        if padded + 1 > mels.shape[1]:                              # (a spectrogram is the longest: the mels grow to its length)
            mels = np.concatenate([mels, np.zeros((mels.shape[0], padded + 1 - mels.shape[1], mels.shape[2]), np.float32)], 1)
        specs = np.zeros((len(spec_List), padded + 1, spec_dim), dtype=np.float32)      # :140-143
        for i, s in enumerate(spec_List):
            specs[i, 1:s.shape[0] + 1] = s
        pattern["teacher_mels"] = mels
        pattern["spectrograms"] = specs
        pattern["spectrogram_lengths"] = np.array([s.shape[0] for s in spec_List], dtype=np.int32)
        return pattern
