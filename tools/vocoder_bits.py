"""A sha256 of what each vocoder writes for every case of tests/{melgan,hifigan,waveglow}_cases.py (HiFi-GAN in its three operand
forms; WaveGlow with the case's fixed z and, again, with fixed seeds): to hold two builds of the library to the same bits.
    python tools/vocoder_bits.py > head.txt;  GSTTACO_LIB=/path/to/other/libgsttaco.so python tools/vocoder_bits.py > other.txt;  diff head.txt other.txt
One process per build.  The hashes are not golden values: tanhf may differ between ROCm releases."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import hifigan_cases, melgan_cases, waveglow_cases      # noqa: E402
from vocoder_harness import Vocoder                      # noqa: E402


def digest(wav, lengths):
    return hashlib.sha256(wav.tobytes() + lengths.tobytes()).hexdigest()


def main():
    for prefix, M, forms in (("melgan", melgan_cases, (None,)), ("hifigan", hifigan_cases, ("float32", "bfloat16", "float16")),
                             ("waveglow", waveglow_cases, (None,))):
        for name in M.NAMES:
            c = M.CASES[name]
            for form in forms:
                v = Vocoder(prefix, c.cfg, c.weights, len(c.frames), c.T, operands=form)
                try:
                    if prefix == "waveglow":
                        print(prefix, name, "z", digest(*v(c.mel, c.frames_array, z=c.z, sigma=c.sigma)))
                        print(prefix, name, "seeds", digest(*v(c.mel, c.frames_array, seeds=range(7, 7 + len(c.frames)), sigma=c.sigma)))
                    else:
                        print(prefix, name, form or "float32", digest(*v(c.mel, c.frames_array)))
                finally:
                    v.close()
        sys.stdout.flush()


if __name__ == "__main__":
    main()
