"""CPU: the inputs of tests/test_gpu_gst.py are well conditioned and can see what they are meant to see (no GPU involved: these are
properties of the cases in tests/gst_cases.py and of the float64 oracle, not of the kernels)."""
import numpy as np
import pytest

import gst_cases as G
from test_gpu_parity import TOL


def _fp32_error(hp, w, mels, lens, ref64):
    return float(np.abs(G.oracle(hp, w, mels, lens, np.float32).astype(np.float64) - ref64).max())


@pytest.mark.parametrize("name", [c.name for c in G.GRID if c.reject is None])
def test_grid_cases_are_well_conditioned(name):
    """A float32 evaluation of the oracle stays within TOL / 5 of the float64 one: the GPU's float32 arithmetic then has room under
    TOL, and an error above TOL is the kernel's.  A case that fails this gets other seeds or sizes, never a wider bound."""
    c = G.GRID_BY_NAME[name]
    ref = G.grid_reference(name)
    err = _fp32_error(c.hp, G.grid_weights(name), *G.inputs(c.shape, c.mel), ref)
    print(name, "oracle float32 against float64: max abs", err, "scale", float(np.abs(ref).max()))
    assert np.isfinite(ref).all() and ref.shape == (c.shape.B, c.hp["GST"]["Style_Token"]["Attention"]["Size"])
    assert err <= TOL / 5


@pytest.mark.parametrize("shape", [G.LONG, G.CAPACITY, G.SHORT, G.SMALL], ids=lambda s: s.name)
def test_full_size_shapes_are_well_conditioned(shape):
    hp, w = G.cfg2_weights()
    ref = G.reference(shape)
    err = _fp32_error(hp, w, *G.inputs(shape), ref)
    print(shape.name, "oracle float32 against float64: max abs", err, "scale", float(np.abs(ref).max()))
    assert err <= TOL / 5


def test_long_case_sees_a_wrong_gather_frame():
    """Shortening one utterance by the stride product -- the neighbouring compressed frame, what a floor instead of a ceil or a pass
    that re-reads the first one would gather -- moves that utterance's embedding by at least 100 x TOL, and no other."""
    hp, w = G.cfg2_weights()
    mels, lens = G.inputs(G.LONG)
    ref = G.reference(G.LONG)
    prod = int(np.prod(hp["GST"]["Reference_Encoder"]["Conv"]["Strides"]))
    assert prod == 64
    assert [int(-(-n // prod) - 1) for n in lens] == [17, 15, 16, 8, 7, 9]
    for b in range(G.LONG.B):
        short = np.array(lens)
        short[b] -= prod
        moved = np.abs(G.oracle(hp, w, mels, short) - ref).max(axis=1)
        print("utterance", b, "length", int(lens[b]), "->", int(short[b]), "moves its embedding by", float(moved[b]))
        assert moved[b] >= 100 * TOL
        assert np.delete(moved, b).max() == 0.0


def test_grid_covers_what_it_claims():
    ok = [c for c in G.GRID if c.reject is None]
    ref = lambda c: c.hp["GST"]["Reference_Encoder"]
    st = lambda c: c.hp["GST"]["Style_Token"]
    assert {ref(c)["RNN"]["Size"] for c in ok} >= {16, 64, 128, 256}
    assert {1024 // (3 * ref(c)["RNN"]["Size"] // 4) for c in ok} >= {85, 21, 10, 5}          # k-parts of the GRU GEMVs
    assert any(ref(c)["Dense"]["Size"] != st(c)["Attention"]["Size"] for c in ok)
    assert {st(c)["Attention"]["Head"] for c in ok} >= {1, 4, 8}
    assert {st(c)["Size"] for c in ok} >= {1, 10, 33}
    assert {c.mel for c in G.GRID} >= {80, 16, 20}
    cins = {cin for c in ok for cin in [1] + ref(c)["Conv"]["Filters"][:-1]}
    assert cins >= {1, 4, 8, 12, 16, 20}
    assert any(len(ref(c)["Conv"]["Filters"]) == 2 for c in ok)
    assert any(1 in ref(c)["Conv"]["Strides"] for c in ok)
    assert any({1, 5} <= set(ref(c)["Conv"]["Kernel_Size"]) for c in ok)
    # every batch has utterances in the second pass of the tail kernel, one of them on its first frame
    for c in G.GRID:
        frames = [-(-int(n) // c.stride_prod) - 1 for n in c.shape.lens]
        assert max(frames) > G.TAIL_MAXT and G.TAIL_MAXT in frames and min(frames) < G.TAIL_MAXT, (c.name, frames)


def test_long_wav_reaches_the_second_pass_after_the_trim():
    """The 9 s signal of the end-to-end test keeps more than 8 x 64 frames once its silent ends are trimmed, and the trim does act."""
    from oracle import audio_np
    hp, _ = G.cfg2_weights()
    snd = hp["Sound"]
    y = G.burst_signal(9.0, snd["Sample_Rate"], seed=1)
    mel = audio_np.mel_generate(np.array(y), snd, 60)
    n = mel.shape[0]
    print("frames after the trim:", n, "of", y.shape[0] // snd["Frame_Shift"], "; lowest mel value", float(mel.min()))
    assert G.TAIL_MAXT * 64 < n < y.shape[0] // snd["Frame_Shift"] - 30
    # no bin at the -100 dB clip (-Max_Abs_Mel), where a float32 front end and the float64 oracle may fall on different sides of it
    short = audio_np.mel_generate(np.array(G.burst_signal(1.5, snd["Sample_Rate"], seed=2)), snd, 60)
    assert mel.min() > -snd["Max_Abs_Mel"] + 0.5 and short.min() > -snd["Max_Abs_Mel"] + 0.5
