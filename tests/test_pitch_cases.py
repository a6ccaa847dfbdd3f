"""CPU checks of tests/pitch_cases.py: the restatement of gsttaco_pitch / gsttaco_pitch_errors gives the answers known in advance, every
case is well conditioned (each decision falls by at least MARGIN relative, in float64 and again in np.longdouble, with the same
outcome), the case table reaches the edges it is meant to reach, and evaluate.combine_pitch / summarize_pitch survive zero denominators.
A case that fails the conditioning test is changed, not excused."""
import numpy as np
import pytest

import audio_cases as C
import pitch_cases as P
from gst_tacotron_amd import evaluate


# ---------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("period", [16, 20, 32, 40])
def test_integer_period_sine_in_float64_is_found_exactly(period):
    """W a multiple of P: d(P) = 0 and d(P-1) = d(P+1) in exact arithmetic, so the parabola's offset is 0 and f0 = sr / P.  The signal is
    float64 here (the float32 rounding of the case table's signals is itself a perturbation of 1e-8)."""
    y = P.sine(400, period, dtype=np.float64)
    W, tau_min, tau_max = 160, 8, 63
    L = W + tau_max
    for u0 in (0, 7, 100):
        f0, ap, lag, off, _ = P.yin_frame(y[u0:u0 + L], W, tau_min, tau_max, 0.1, 16000)
        assert lag == period and abs(f0 - 16000.0 / period) <= 1e-9 * 16000.0 / period, (f0, off)
        assert ap < 1e-12


@pytest.mark.parametrize("name", ["sine_integer_periods", "sine_between_periods", "harmonic_complexes", "default_321_lags"])
def test_interior_frames_find_the_period(name):
    """Every frame whose span lies inside the signal is voiced at the signal's period: within 1e-6 for integer periods (float32 samples),
    within 1 % between them and for the complexes -- whose first dip under the threshold must be the period's, not the half period's."""
    c = P.CASES[name]
    for row, period in c.expect.items():
        ref = P.case_reference(name)[row]
        inner = P.interior_frames(ref, c)
        assert inner.size >= 3, (name, row)
        f0 = ref["f0"][inner]
        tol = 1e-6 if name == "sine_integer_periods" else 1e-2
        assert (np.abs(f0 - c.sound.sr / period) <= tol * c.sound.sr / period).all(), (name, row, f0, c.sound.sr / period)


def test_noise_and_silence_are_unvoiced_and_the_mixed_row_is_both():
    noise, silence = P.case_reference("noise_and_silence")
    assert noise["frames"] > 20 and (noise["lag"] == 0).all() and (noise["f0"] == 0).all() and (noise["aperiodicity"] > 0.3).all()
    assert (silence["lag"] == 0).all() and (silence["aperiodicity"] == 1.0).all()        # d' = 1 over digital silence
    mixed = P.case_reference("voiced_between_noise")[0]
    voiced = mixed["lag"] > 0
    t = np.arange(mixed["frames"]) * P.TINY.hop
    assert voiced[(t > 420) & (t < 700)].all() and not voiced[t < 200].any() and not voiced[t > 920].any()
    assert (np.abs(mixed["f0"][(t > 420) & (t < 700)] - 640.0) < 6.4).all()


def test_the_table_reaches_the_edges_it_names():
    nl = lambda c: P.lag_range(c.sound.sr, c.fmin, c.fmax)[1] + 1
    assert [nl(P.CASES["lags_%d" % k]) for k in (63, 64, 65)] == [63, 64, 65]
    d = P.CASES["default_321_lags"]
    assert nl(d) == 321 and P.window_of(d.sound.sr, d.window) == 400 and P.lag_range(16000, 50.0, 500.0) == (32, 320)
    assert P.CASES["odd_window"].window % 2 == 1 and P.CASES["span_at_lds_limit"].span == 3071
    frames = [r["frames"] for r in P.case_reference("length_edges")]
    assert frames == [0, 1 + (P.H + 1) // P.HOP, 11, 10]
    ragged = [r["frames"] for r in P.case_reference("ragged_batch")]
    assert ragged[1] == 0 and len(set(ragged)) == len(ragged)
    for top_db in C.TOP_DBS:                                            # the trimmed rows have the front end's frame counts
        c = P.CASES["trim_%d" % top_db]
        got = [r["frames"] for r in P.case_reference(c.name)]
        assert got == [C.expected_frames(c.sound, w, top_db) for w in c.rows] and 0 in got and max(got) > 10
    assert [r["frames"] for r in P.case_reference("no_trim")] != [r["frames"] for r in P.case_reference("trim_60")]
    for name in P.NAMES:                                                # every case but the silent rows has voiced and unvoiced material
        assert sum(r["frames"] for r in P.case_reference(name)) > 0
    assert any((r["lag"] > 0).any() for r in P.case_reference("trim_15"))


def test_fastvox_frames_equal_the_stored_mels_and_the_voices_are_plausible():
    """The seven FastVox references at the defaults with top_db 15: frame t of the track is frame t of the stored mel, and the median F0 of
    each voice lies where a human voice does."""
    g = np.load(P.GOLD + "/audio_fv_all.npz")
    refs = P.case_reference("fastvox_defaults")
    medians = []
    for i, r in enumerate(refs):
        assert r["frames"] == g["mel%d" % i].shape[0] and (r["start"], r["start"] + r["n"]) == tuple(g["bounds%d" % i])
        voiced = r["f0"][r["lag"] > 0]
        assert voiced.size >= 20
        medians.append(float(np.median(voiced)))
    print("FastVox median F0 per voice:", np.round(medians, 1))
    assert all(70.0 < m < 260.0 for m in medians)


# ---------------------------------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("name", P.NAMES)
def test_every_decision_of_a_case_is_decided_by_the_margin(name):
    """Each d'(tau) against the threshold, each comparison down the dip and each parabola denominator (against a + c) falls by at least
    MARGIN relative -- in float64 and in np.longdouble, with the same voiced set and lags -- so a device that differs from the
    restatement by rounding alone takes every decision the same way."""
    r64, r80 = P.case_reference(name), P.case_reference(name, np.longdouble)
    smallest = 1.0
    for a, b in zip(r64, r80):
        assert a["frames"] == b["frames"] and np.array_equal(a["lag"], b["lag"])
        if a["frames"]:
            smallest = min(smallest, a["margin"].min(), b["margin"].min())
            assert np.allclose(a["f0"], b["f0"], rtol=1e-9, atol=0) and np.allclose(a["aperiodicity"], b["aperiodicity"], rtol=1e-9, atol=0)
    print(name, "smallest decision margin", smallest)
    assert smallest >= P.MARGIN


@pytest.mark.parametrize("name", P.ERROR_NAMES)
def test_error_cases_are_decided_and_read_off_by_inspection(name):
    c = P.ERROR_CASES[name]
    counts, sums, margin = P.error_reference(name)
    counts80, sums80, margin80 = P.error_reference(name, np.longdouble)
    assert np.array_equal(counts, counts80) and np.allclose(sums, sums80, rtol=1e-12, atol=0) and min(margin, margin80) >= P.MARGIN
    if c.counts is not None:
        assert np.array_equal(counts, c.counts)
    assert (counts[:, 1] + counts[:, 3] <= counts[:, 0]).all() and (counts[:, 2] <= counts[:, 1]).all()
    assert np.array_equal(counts[:, 4] + counts[:, 5], 2 * counts[:, 1] + counts[:, 3])


def test_error_cases_cover_the_pairing_rules():
    by = {n: P.error_reference(n)[0] for n in P.ERROR_NAMES}
    assert by["diagonal_unequal_lengths"][:, 0].tolist() == [33, 12, 0]                 # min(Lx, Ly)
    stairs, holes = by["staircase_paths"], by["paths_with_holes"]
    assert stairs[:, 0].tolist() == P.ERROR_CASES["staircase_paths"].path_len.tolist()
    assert holes[:, 0].tolist() == [stairs[0, 0] - 4, stairs[1, 0] - 1, stairs[2, 0] - 1]   # -1 rows and outside cells are skipped
    assert (by["zero_length_rows"] == 0).all() and (P.error_reference("zero_length_rows")[1] == 0).all()
    assert P.error_reference("by_inspection")[1][0, 0] == 1200 * np.log2(119 / 100.0)   # (100, 100) adds 0


# ---------------------------------------------------------------------------------------------------- the host side
def test_combine_and_summarize_pitch():
    counts = np.array([[10, 6, 2, 3, 8, 7], [0, 0, 0, 0, 0, 0], [4, 0, 0, 4, 4, 0], [5, 5, 5, 0, 5, 5]], np.int32)
    sums = np.array([[40.0, 500.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
    per = evaluate.combine_pitch(counts, sums)
    assert per.shape == (4, len(evaluate.PITCH_FIELDS)) and per.dtype == np.float64 and np.isfinite(per).all()
    f = evaluate.PITCH_FIELDS.index
    assert per[0, f("gpe")] == 2 / 6 and per[0, f("vde")] == 0.3 and per[0, f("ffe")] == 0.5
    assert per[0, f("f0_mae_cents")] == 10.0 and per[0, f("f0_rmse_cents")] == np.sqrt(125.0) and per[0, f("voiced_ratio")] == 8 / 7
    assert per[0, f("pairs")] == 10 and per[0, f("both_voiced")] == 6
    assert (per[1] == 0).all()                                          # every denominator zero: 0, not NaN
    assert per[2, f("gpe")] == 0 and per[2, f("vde")] == 1 and per[2, f("voiced_ratio")] == 0
    assert per[3, f("gpe")] == 1 and per[3, f("f0_mae_cents")] == 0 and per[3, f("f0_rmse_cents")] == 0     # all gross: no cents
    s = evaluate.summarize_pitch(counts, sums)
    assert s["gpe"] == per[:, 0].mean() and s["vde"] == per[:, 1].mean() and s["ffe"] == per[:, 2].mean()
    assert s["gpe_frames"] == 7 / 11 and s["vde_frames"] == 7 / 19 and s["ffe_frames"] == 14 / 19
    empty = evaluate.summarize_pitch(counts[1:2], sums[1:2])
    assert all(v == 0.0 for v in empty.values())
    with pytest.raises(ValueError):
        evaluate.combine_pitch(counts[:, :5], sums)
