"""CPU checks of tests/report_cases.py (the NumPy restatements the GPU tests of csrc/report.hip compare against), of the host
bookkeeping behind Inference_Checked (gst_tacotron_amd/checked.py) and of the new surface: two C-ABI symbols, the ``seeds`` keyword."""
import inspect
import os
import re

import numpy as np
import pytest

import report_cases as R
from gst_tacotron_amd import checked
from oracle import rng_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(rep, b=0):
    return dict(zip(R.FIELDS, rep[b].tolist()))


# ---------------------------------------------------------------------------------------------------- the report restatement
def test_report_of_a_hand_written_path():
    path = [0, 0, 1, 3, 3, 3, 2, 5]
    align = R.one_hot_path(path, 6)
    stop = np.ones((1, 8), np.float32)
    rep, focus = R.report(stop, align, 2)
    assert rep.dtype == np.int32 and rep.shape == (1, 8)
    assert _row(rep) == dict(stop_step=8, frames=16, end_gap=0, max_jump=3, back_steps=1, max_stall=3, visited=5, nonfinite=0)
    assert abs(focus[0] - np.float64(np.float32(0.9))) < 1e-15
    # the stop fires at step 6: the back step (5 -> 6) and the jump to token 5 lie behind it
    stop[0, 6] = -0.5
    rep, _ = R.report(stop, align, 2)
    assert _row(rep) == dict(stop_step=6, frames=12, end_gap=2, max_jump=2, back_steps=0, max_stall=3, visited=3, nonfinite=0)
    # a longer text than the attention walked: Tv 9, the last token reached is 5
    rep, _ = R.report(np.ones((1, 8), np.float32), R.one_hot_path(path, 9), 3)
    assert _row(rep)["end_gap"] == 3 and _row(rep)["frames"] == 24
    # token_lengths cut the columns: below 4 tokens the argmax cannot be 5 or 3
    rep, _ = R.report(np.ones((1, 8), np.float32), align, 2, token_lengths=[3])
    r3 = _row(rep)
    assert r3["end_gap"] == 0 and r3["visited"] <= 3 and r3["max_jump"] <= 2


def test_report_stop_edges():
    align = R.one_hot_path([0, 1, 2, 2], 3)
    # s* = 0: one step is still looked at, one step's frames are still emitted (Model.py:413 max(1, .))
    rep, focus = R.report(np.array([[-1.0, 1.0, -1.0, 1.0]], np.float32), align, 2)
    assert _row(rep) == dict(stop_step=0, frames=2, end_gap=2, max_jump=0, back_steps=0, max_stall=1, visited=1, nonfinite=0)
    assert abs(focus[0] - np.float64(np.float32(0.9))) < 1e-15
    # no stop at all; 0.0 is not negative
    rep, _ = R.report(np.array([[0.0, 1.0, 2.0, 0.0]], np.float32), align, 2)
    assert _row(rep) == dict(stop_step=4, frames=8, end_gap=0, max_jump=1, back_steps=0, max_stall=2, visited=3, nonfinite=0)
    # a NaN is not below 0 -- and counts as non-finite when it lies before the stop
    rep, _ = R.report(np.array([[np.nan, 1.0, -2.0, np.nan]], np.float32), align, 2)
    assert _row(rep)["stop_step"] == 2 and _row(rep)["frames"] == 4 and _row(rep)["nonfinite"] == 1
    # n = 1 (also from a token length of 0, clipped): the attention cannot move
    rep, focus = R.report(np.ones((1, 4), np.float32), align, 1, token_lengths=[0])
    assert _row(rep) == dict(stop_step=4, frames=4, end_gap=0, max_jump=0, back_steps=0, max_stall=4, visited=1, nonfinite=0)
    assert abs(focus[0] - align[0, :, 0].astype(np.float64).mean()) < 1e-15


def test_report_counts_non_finite_values_only_in_front_of_the_stop():
    align = R.one_hot_path([0, 1, 1, 2], 4)
    stop = np.array([[1.0, 1.0, -1.0, 1.0]], np.float32)       # s* = 2, frames = 6 at r = 3
    mel = np.zeros((1, 12, 5), np.float32)
    mel[0, 5, 4] = np.inf                                       # frame frames - 1: counted
    mel[0, 6, 0] = np.inf                                       # frame frames: not counted
    align[0, 3, 0] = np.nan                                     # step 3 >= E: not counted
    rep, _ = R.report(stop, align, 3, mel=mel)
    assert _row(rep)["nonfinite"] == 1 and _row(rep)["frames"] == 6
    align[0, 1, 3] = -np.inf                                    # step 1 < E, column 3 < n = 4: counted; with n = 3 it is not
    assert _row(R.report(stop, align, 3, mel=mel)[0])["nonfinite"] == 2
    assert _row(R.report(stop, align, 3, token_lengths=[3], mel=mel)[0])["nonfinite"] == 1


def test_report_ties_take_the_lowest_index():
    align = np.zeros((1, 2, 150), np.float32)
    align[0, 0, [70, 5, 133]] = 1.0
    align[0, 1, [149, 64]] = 2.0
    rep, focus = R.report(np.ones((1, 2), np.float32), align, 1)
    assert _row(rep)["max_jump"] == 59 and _row(rep)["end_gap"] == 149 - 64 and focus[0] == 1.5


# ---------------------------------------------------------------------------------------------------- the seeded randomness
SEEDS = [(0xDEADBEEF << 32) | 17, (1 << 63) + 5, 0xFFFFFFFFFFFFFFFF]


@pytest.mark.parametrize("rate", [0.5, 0.25])
def test_randomness_depends_on_the_seed_alone(rate):
    steps, P = 3, 64
    m70, n70 = R.randomness(SEEDS, steps, 70, P, rate)
    m12, n12 = R.randomness(SEEDS, steps, 12, P, rate)
    assert m70.shape == (steps, 2, 3, P) and m70.dtype == np.float32 and n70.shape == (steps, 3, 70)
    assert np.array_equal(m70, m12) and np.array_equal(n70[:, :, :12], n12)                    # not on Tv
    order = [2, 0, 1]
    mp, npm = R.randomness([SEEDS[i] for i in order], steps, 70, P, rate)
    assert np.array_equal(mp, m70[:, :, order]) and np.array_equal(npm, n70[:, order])         # not on the row
    one_m, one_n = R.randomness(SEEDS[1:2], steps, 70, P, rate)
    assert np.array_equal(one_m[:, :, 0], m70[:, :, 1]) and np.array_equal(one_n[:, 0], n70[:, 1])      # not on B
    # it IS the single-seed tensor of a batch of one, and it is NOT row b of the single-seed batch
    assert np.array_equal(one_m.reshape(steps, -1), rng_np.masks(SEEDS[1], steps, 1, P, P, rate))
    whole = rng_np.masks(SEEDS[1], steps, 3, P, P, rate).reshape(steps, 2, 3, P)
    assert np.array_equal(whole[:, :, 0], one_m[:, :, 0]) and not np.array_equal(whole[:, :, 1], one_m[:, :, 0])
    assert set(np.unique(m70)) == {0.0, 1.0} and abs(m70.mean() - (1.0 - rate)) < 0.05
    assert not np.array_equal(m70[:, :, 0], m70[:, :, 1])


# ---------------------------------------------------------------------------------------------------- Inference_Checked's bookkeeping
def test_attempt_seeds_wrap_mod_2_64():
    assert checked.attempt_seed(5, 0) == 5
    assert checked.attempt_seed(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert checked.attempt_seed(5, 2) == (5 + 2 * 0x9E3779B97F4A7C15) % (1 << 64) == 5 + 0x3C6EF372FE94F82A
    assert checked.attempt_seed((1 << 64) - 1, 1) == 0x9E3779B97F4A7C14
    assert checked.attempt_seed(-1, 0) == (1 << 64) - 1 and checked.attempt_seed(1 << 64, 0) == 0


def test_run_checked_reruns_only_the_rejected_rows_and_scatters_them_back():
    seeds = [10, (1 << 64) - 3, 30, 40]
    reject = {(0, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)}   # (utterance, attempt); utterance 3 is never accepted
    calls, store, judged = [], {}, []

    def run(rows, row_seeds):
        calls.append((list(rows), list(row_seeds)))
        for i, s in zip(rows, row_seeds):
            store[i] = s                                        # what an attempt "synthesised": its seed
        return [[i, len(calls)] for i in rows], [float(i) for i in rows]

    def accept(row, focus, i, k):
        judged.append((i, k))
        assert row == [i, k + 1] and focus == float(i)
        return (i, k) not in reject

    attempts, accepted = checked.run_checked(seeds, 3, run, accept)
    assert attempts == [1, 0, 2, 2] and accepted == [True, True, True, False]
    assert [c[0] for c in calls] == [[0, 1, 2, 3], [0, 2, 3], [2, 3]]
    G = 0x9E3779B97F4A7C15
    assert calls[0][1] == seeds
    assert calls[1][1] == [10 + G, 30 + G, 40 + G] and calls[2][1] == [(30 + 2 * G) % (1 << 64), (40 + 2 * G) % (1 << 64)]
    assert store == {i: checked.attempt_seed(seeds[i], k) for i, k in enumerate(attempts)}     # the last attempt's outputs stay
    assert judged == [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (2, 1), (3, 1), (2, 2), (3, 2)]
    # everything accepted at once: one call; max_attempts = 1: one call whatever accept says
    calls.clear()
    assert checked.run_checked(seeds, 3, run, lambda *a: True) == ([0] * 4, [True] * 4) and len(calls) == 1
    calls.clear()
    assert checked.run_checked(seeds, 1, run, lambda *a: False) == ([0] * 4, [False] * 4) and len(calls) == 1
    with pytest.raises(ValueError):
        checked.run_checked(seeds, 0, run, accept)


def test_default_accept_is_stop_fired_text_finished_all_finite():
    ok = checked.default_accept(13)
    row = dict(stop_step=7, frames=14, end_gap=0, max_jump=9, back_steps=4, max_stall=6, visited=2, nonfinite=0)
    as_row = lambda **kw: [dict(row, **kw)[f] for f in checked.REPORT_FIELDS]
    assert checked.REPORT_FIELDS == R.FIELDS
    assert ok(as_row(), 0.1, 0, 0)
    assert not ok(as_row(stop_step=13), 0.9, 0, 0) and not ok(as_row(end_gap=1), 0.9, 0, 0) and not ok(as_row(nonfinite=2), 0.9, 0, 0)


# ---------------------------------------------------------------------------------------------------- the surface
NEW_SYMBOLS = ("gsttaco_fill_randomness", "gsttaco_utterance_report")


def test_abi_declares_the_report_entry_points_and_is_still_14():
    from gst_tacotron_amd import build, capi
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    assert re.search(r"#define\s+GSTTACO_ABI_VERSION\s+14\b", header) and capi.ABI_VERSION == 14
    src = open(os.path.join(ROOT, "gst_tacotron_amd", "csrc", "gsttaco.cpp")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert re.search(r"\bint\s+" + sym + r"\s*\(", src), sym
        assert sym in capi.EXPORTED_SYMBOLS, sym
    assert "report.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "gst_tacotron_amd", "csrc", "report.hip"))
    kernels_h = open(os.path.join(ROOT, "gst_tacotron_amd", "csrc", "kernels.h")).read()
    assert "gt_launch_fill_randomness" in kernels_h and "gt_launch_utterance_report" in kernels_h


def test_python_surface_has_seeds_and_the_report():
    from gst_tacotron_amd import model
    from gst_tacotron_amd.model import GST_Tacotron
    for fn in (GST_Tacotron.Inference_Step, GST_Tacotron.decode, GST_Tacotron.Inference, GST_Tacotron.Inference_GTA):
        assert inspect.signature(fn).parameters["seeds"].default is None, fn
    sig = inspect.signature(GST_Tacotron.Utterance_Report).parameters
    assert list(sig)[1:] == ["stops", "alignments", "token_lengths", "mels"] and sig["token_lengths"].default is None
    sig = inspect.signature(GST_Tacotron.Inference_Checked).parameters
    assert list(sig)[1:9] == ["sentence_List", "wav_List_for_GST", "style_embeddings", "style_token_weights", "seeds", "max_attempts",
                              "accept", "export"]
    assert sig["max_attempts"].default == 3 and sig["accept"].default is None and sig["export"].default is False
    assert model.REPORT_FIELDS == R.FIELDS and len(model.REPORT_FIELDS) == 8
    assert "capture_after=2" in GST_Tacotron.Inference_Checked.__doc__
