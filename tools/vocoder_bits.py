"""A sha256 of what each vocoder writes for every case of tests/{melgan,hifigan,waveglow}_cases.py (HiFi-GAN in its three operand
forms; WaveGlow with the case's fixed z and, again, with fixed seeds), and then for every row of the size surface
(tests/vocoder_surface_cases.py: uneven wave items, shrunk tiles, the launches at the LDS bound, kc 64 / 16): to hold two builds of
the library to the same bits.
    python tools/vocoder_bits.py > head.txt;  GSTTACO_LIB=/path/to/other/libgsttaco.so python tools/vocoder_bits.py > other.txt;  diff head.txt other.txt
One process per build.  The hashes are not golden values: tanhf may differ between ROCm releases.  The case tables come first and
print what they printed before the surface was added."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import hifigan_cases, melgan_cases, vocoder_surface_cases, waveglow_cases      # noqa: E402
from vocoder_harness import Vocoder                      # noqa: E402

FORMS = {"melgan": (None,), "hifigan": ("float32", "bfloat16", "float16"), "waveglow": (None,)}


def digest(wav, lengths):
    return hashlib.sha256(wav.tobytes() + lengths.tobytes()).hexdigest()


def case_bits(prefix, c, tag):
    """the lines of one case (a module's Case) in every operand form of its module"""
    for form in FORMS[prefix]:
        v = Vocoder(prefix, c.cfg, c.weights, len(c.frames), c.T, operands=form)
        try:
            if prefix == "waveglow":
                print(tag, c.name, "z", digest(*v(c.mel, c.frames_array, z=c.z, sigma=c.sigma)))
                print(tag, c.name, "seeds", digest(*v(c.mel, c.frames_array, seeds=range(7, 7 + len(c.frames)), sigma=c.sigma)))
            else:
                print(tag, c.name, form or "float32", digest(*v(c.mel, c.frames_array)))
        finally:
            v.close()


def main():
    for prefix, M in (("melgan", melgan_cases), ("hifigan", hifigan_cases), ("waveglow", waveglow_cases)):
        for name in M.NAMES:
            case_bits(prefix, M.CASES[name], prefix)
        sys.stdout.flush()
    for name in vocoder_surface_cases.NAMES:
        r = vocoder_surface_cases.ROWS[name]
        case_bits(r.module, r.case, "surface " + r.module)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
