"""CPU checks of tests/forced_cases.py (the float64 teacher-forced decoder the GPU tests compare against) and of the host side of
teacher forcing: the durations count, the Feeder's teacher layout, the three new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

import forced_cases as F
from gst_tacotron_amd import synthetic
from oracle import oracle_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_run(shape, seed):
    c = F.make_case(shape, seed)
    w64 = oracle_np.cast_weights(c.w, np.float64)
    return c, oracle_np.decoder(c.hp, w64, c.memory, np.float64, c.masks.astype(np.float64), c.noise.astype(np.float64), steps=c.S)


@pytest.mark.parametrize("shape", F.CPU, ids=lambda s: "{}-r{}".format(s.att, s.r))
def test_forced_on_the_free_runs_own_frames_is_the_free_run(shape):
    """Teacher = the oracle's own free-run pre_mel behind a zero frame: the forced restatement consumes exactly the frames the free
    run fed back, so it must BE oracle_np.decoder (measured: exactly 0.0 for all three outputs)."""
    c, (pre, stop, align) = _free_run(shape, 100 + shape.r)
    got = F.reference(c, teacher=F.behind_go_frame(pre))
    errs = [np.abs(g - e).max() for g, e in zip(got, (pre, stop, align))]
    print(shape, "forced on own frames vs free run", errs)
    assert got[0].shape == (shape.B, c.S * shape.r, 80) and c.S == 8
    assert max(errs) <= 1e-12, errs


@pytest.mark.parametrize("shape", F.CPU, ids=lambda s: "{}-r{}".format(s.att, s.r))
def test_forced_restatement_is_well_conditioned_and_sees_a_shifted_teacher(shape):
    """float32 against float64 on a clipped-normal teacher (measured on these cases: at most 8.2e-7; a fifth of the bar leaves the
    kernels four fifths), and a teacher that arrives one frame early moves every output by far more than the bar (measured: at least
    0.15 / 0.044 / 0.017 for pre-mel / stop / alignment, against 100 x TOL = 0.005)."""
    c = F.make_case(shape, 200 + shape.r)
    ref = F.reference(c)
    f32 = F.reference(c, dt=np.float32)
    errs = [np.abs(a.astype(np.float64) - b).max() for a, b in zip(f32, ref)]
    print(shape, "float32 vs float64", errs)
    assert all(a.dtype == np.float32 for a in f32)
    assert max(errs) <= F.TOL / 5, errs
    early = np.concatenate([c.teacher[:, 1:], c.teacher[:, -1:]], 1)         # step t consumes frame t * r + 1
    moved = [np.abs(a - b).max() for a, b in zip(F.reference(c, teacher=early), ref)]
    print(shape, "teacher one frame early moves", moved)
    assert min(moved) >= 100 * F.TOL, moved


def test_durations_rows_sum_to_the_length_and_the_lowest_index_wins_ties():
    rng = np.random.default_rng(5)
    B, S, Tv, r = 4, 7, 11, 3
    align = rng.random((B, S, Tv)).astype(np.float32)
    align[0, 2, :] = 0.25                       # a whole row tied: token 0
    align[1, 3, 4] = align[1, 3, 9] = 2.0       # a two-way tie: token 4
    align[2, 0, 9] = 3.0                        # beyond token_lengths[2]: not counted there
    tl, ml = np.array([11, 10, 6, 1]), np.array([21, 20, 5, 40])
    d = F.durations(align, r, tl, ml)
    assert d.dtype == np.int32 and d.shape == (B, Tv)
    assert d.sum(1).tolist() == [21, 20, 5, 21]                              # min(mel_length, S * r)
    assert d[0, 0] >= 3 and d[1, 4] >= 3 and not d[2, 6:].any() and d[3, 0] == 21
    full = F.durations(align, r)
    assert full.sum(1).tolist() == [S * r] * B and full[2, 9] >= 3
    assert F.durations(align, r, None, np.array([1, 2, 3, 4])).sum(1).tolist() == [1, 2, 3, 4]      # lengths that are no multiple of r


@pytest.mark.parametrize("r", [1, 2, 3])
def test_teacher_pattern_has_the_reference_feeders_layout(r):
    from gst_tacotron_amd.feeder import Feeder
    hp = synthetic.config_hp("cfg2")
    hp["Step_Reduction"] = r
    rng = np.random.default_rng(r)
    mels = [rng.normal(size=(n, 80)).astype(np.float32) for n in (7, 12, 1)]
    sentences = ["Hello.", "A longer sentence", "x"]
    f = Feeder(hp)
    p = f.Get_Teacher_Pattern(sentences, mels)
    want = F.teacher_layout(mels, r, 80)
    assert p["teacher_mels"].dtype == np.float32 and np.array_equal(p["teacher_mels"], want)
    Tq = want.shape[1]
    assert (Tq - 1) % r == 0 and Tq - 1 >= 13 and not want[:, 0].any() and not want[:, -1].any()
    assert F.n_steps(Tq, r) * r == Tq - 1                                    # every target frame is emitted
    assert p["mel_lengths"].tolist() == [7, 12, 1] and p["mel_lengths"].dtype == np.int32
    inf = f.Get_Inference_Pattern(sentences, style_given=True)
    assert np.array_equal(p["tokens"], inf["tokens"]) and np.array_equal(p["token_lengths"], inf["token_lengths"])
    assert "initial_mels" not in p
    with pytest.raises(ValueError):
        f.Get_Teacher_Pattern(sentences, mels[:2])


def test_abi_declares_the_forced_entry_points_and_is_still_14():
    from gst_tacotron_amd import capi
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    assert re.search(r"#define\s+GSTTACO_ABI_VERSION\s+14\b", header) and capi.ABI_VERSION == 14
    for sym in ("gsttaco_decode_forced", "gsttaco_inference_step_forced", "gsttaco_forced_durations"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in capi.EXPORTED_SYMBOLS, sym
    src = open(os.path.join(ROOT, "gst_tacotron_amd", "csrc", "gsttaco.cpp")).read()
    for sym in ("gsttaco_decode_forced", "gsttaco_inference_step_forced", "gsttaco_forced_durations"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", src), sym


def test_python_surface_has_the_teacher_arguments():
    import inspect
    from gst_tacotron_amd.model import GST_Tacotron
    for fn in (GST_Tacotron.Inference_Step, GST_Tacotron.decode):
        assert inspect.signature(fn).parameters["teacher_mels"].default is None
    for name in ("Forced_Durations", "Inference_GTA"):
        assert callable(getattr(GST_Tacotron, name))
