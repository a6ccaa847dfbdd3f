"""CPU checks of tests/saturated_cases.py: every case the GPU tests compare on is admitted by the oracle alone and is in the regime its
recipe names, the ill-conditioned BMA case is rejected, the Glorot baseline shows none of the regime, the traced decoder IS the
oracle's, and a control -- the score pass with hoisted exponentials -- passes at Glorot scale and fails on "sma_wide"."""
import numpy as np
import pytest

import saturated_cases as S
from oracle import oracle_np


@pytest.mark.parametrize("name", S.ADMITTED)
def test_every_case_is_admitted_and_in_its_regime(name):
    c, m = S.measured(name)
    print(S.describe(name, m))
    assert S.admit(m, S.CONDITIONS[name]) == []
    assert all(np.isfinite(v).all() for v in m["ref"].values())
    assert m["shares"]["enc_h_eq_1"] > 0                       # (the encoder BiLSTM's biases are saturated in every recipe)
    if c.token_lengths is not None:
        for b, n in enumerate(c.token_lengths):
            assert not m["ref"]["align"][b][:, n:].any() and not m["ref"]["encoder"][b, n:].any()
        assert 1 in c.token_lengths.tolist() and c.spec.Tv in c.token_lengths.tolist()


def test_sma_sharp_alignment_is_one_hot_and_walks():
    _, m = S.measured("sma_sharp")
    path = m["shares"]["argmax_path"][0]
    assert (np.diff(path) >= 0).all() and (np.diff(path) <= 1).all() and path[-1] - path[0] >= 4, path
    assert m["shares"]["max_align"] > 1 - 1e-6


def test_the_ill_conditioned_bma_case_is_rejected():
    """score_bias 25 over 10 steps: float32 and float64 of Steps.py's safe-cumprod part ways, by orders more than the admission allows
    -- the regime conditions themselves hold, the floor alone rejects it."""
    _, m = S.measured("bma_bias25")
    print(S.describe("bma_bias25", m))
    why = S.admit(m, S.CONDITIONS["bma_bias25"])
    assert why and all(r.startswith("floor of") for r in why), why
    assert m["floor"]["align"] > 100 * S.ADMIT / S.FLOOR_FACTOR


def test_the_glorot_baseline_shows_none_of_the_regime():
    """The helper's honesty: on the suite's own weights no gate is beyond |z| = 8, no p beyond 1 - 1e-4, no encoder state +-1.0f,
    so every decoder recipe's conditions REJECT it -- and so do they reject each case with ``trained_like`` made the identity."""
    _, m = S.measured("glorot")
    s = m["shares"]
    print(S.describe("glorot", m))
    assert s["z_gt_8"] == 0 and s["max_z"] < 4 and s["p_gt_1-1e-4"] == 0 and s["one_minus_p_lt_6e-8"] == 0 and s["p_lt_1e-4"] < 0.01
    assert s["enc_h_eq_1"] == 0 and s["max_tanh_arg"] < 8
    assert S.admit(m, ()) == []                                 # (well conditioned, of course)
    for name in S.ADMITTED:
        assert S.admit(m, S.CONDITIONS[name]), name
    c = S.make_case("sma_wide", identity=True)
    assert all(np.array_equal(c.w[k], S.make_case("glorot").w[k]) for k in c.w)
    assert S.admit(S.measure(c), S.CONDITIONS["sma_wide"])


def test_trained_like_changes_what_it_says_and_nothing_else():
    hp, w0 = S.recipe_weights("sma_sharp", identity=True)
    _, w = S.recipe_weights("sma_sharp")
    r = S.RECIPES["sma_sharp"]
    changed = {k for k in w if not np.array_equal(w[k], w0[k])}
    lstm = {k for k in w if S._is_lstm_bias(k)}
    assert len(lstm) == 6 and lstm <= changed
    highway = {k for k in w if S._is_highway_bias(k)}
    assert len(highway) == 2 * int(hp["Vocoder_Taco1"]["CBHG"]["Highwaynet"]["Count"]) and highway <= changed
    scaled = {"decoder.lstm0.kernel": r.g_k, "decoder.lstm0.recurrent_kernel": r.g_k, "decoder.lstm1.kernel": r.g_k,
              "decoder.lstm1.recurrent_kernel": r.g_k, "decoder.attention.v": r.g_v, "decoder.attention.value.kernel": r.g_m,
              "decoder.attention.query.kernel": r.g_q}
    for k, g in scaled.items():
        assert np.array_equal(w[k], (w0[k] * np.float32(g)).astype(np.float32)), k
    assert float(w["decoder.attention.score_bias"]) == r.score_bias
    assert changed == lstm | highway | set(scaled) | {"decoder.attention.score_bias"}
    sd = np.concatenate([(w[k] - w0[k]).ravel() for k in sorted(lstm | highway)]).std()
    assert abs(sd - r.sigma_b) < 0.05 * r.sigma_b
    assert all(v.dtype == np.float32 for v in w.values()) and w0["decoder.attention.v"] is not w["decoder.attention.v"]
    _, wl0 = S.recipe_weights("lsa_sharp", identity=True)
    _, wl = S.recipe_weights("lsa_sharp")
    assert 2.5 < (wl["decoder.attention.bias"] - wl0["decoder.attention.bias"]).std() < 3.5
    _, we = S.recipe_weights("encoder")
    assert {k for k in we if not np.array_equal(we[k], w0[k])} == lstm | highway


@pytest.mark.parametrize("name", ["sma_sharp", "bma", "lsa_sharp", "sma_long_masked"])
def test_the_traced_decoder_is_the_oracles_decoder(name):
    c, m = S.measured(name)
    w64 = oracle_np.cast_weights(c.w, np.float64)
    mem = oracle_np.gst_concat(m["ref"]["encoder"], m["ref"]["gst"])
    ref = oracle_np.decoder(c.hp, w64, mem, np.float64, c.masks.astype(np.float64), c.noise.astype(np.float64), steps=c.spec.steps,
                            token_lengths=c.token_lengths)
    for k, r in zip(("pre_mel", "stop", "align"), ref):
        assert np.array_equal(m["ref"][k], r), k
    w32 = oracle_np.cast_weights(c.w, np.float32)
    old = np.seterr(over="ignore")
    try:
        ref32 = oracle_np.decoder(c.hp, w32, mem.astype(np.float32), np.float32, c.masks, c.noise, steps=c.spec.steps,
                                  token_lengths=c.token_lengths)
    finally:
        np.seterr(**old)
    for k, r in zip(("pre_mel", "stop", "align"), ref32):
        assert r.dtype == np.float32 and np.array_equal(m["f32"][k], r), k


def test_end_to_end_reference_is_oracle_inference_step():
    c, m = S.measured("sma_sharp")
    ref = oracle_np.inference_step(c.hp, c.w, c.tokens, c.mels, c.mel_lengths, c.masks, c.noise, steps=c.spec.steps, dt=np.float64,
                                   with_vocoder=True)
    assert np.array_equal(ref[0], m["ref"]["mel"]) and np.array_equal(ref[2], m["ref"]["spectrogram"])
    assert np.array_equal(ref[1], m["ref"]["stop"]) and np.array_equal(ref[3], m["ref"]["align"])


def _hoisted_float32(name):
    """The float32 decoder with the control's score pass against the case's float64 reference: per-output error (inf: non-finite)."""
    c, m = S.measured(name)
    mem = oracle_np.gst_concat(m["ref"]["encoder"], m["ref"]["gst"]).astype(np.float32)
    old = np.seterr(over="ignore", invalid="ignore")
    try:
        got = S.traced_decoder(c.hp, oracle_np.cast_weights(c.w, np.float32), mem, np.float32, c.masks, c.noise, c.spec.steps,
                               c.token_lengths, score_fn=S.hoisted_score)
    finally:
        np.seterr(**old)
    errs = {k: S._err(g, m["ref"][k]) for k, g in zip(("pre_mel", "stop", "align"), got)}
    return errs, {k: S.tolerance(m["floor"][k]) for k in errs}


def test_control_hoisted_exponentials_pass_at_glorot_scale_and_fail_on_sma_wide():
    """The cases can fail.  tanh(q + m) = (E_q E_m - 1) / (E_q E_m + 1) is a correct form at Glorot scale -- the suite as it was could
    not tell it from the kernels' -- and is NaN or far off where |q + m| passes 44.4: the comparison the GPU tests make sees it."""
    errs, tol = _hoisted_float32("glorot")
    print("hoisted form, glorot", errs, tol)
    assert all(errs[k] <= tol[k] for k in errs), errs
    errs, tol = _hoisted_float32("sma_wide")
    print("hoisted form, sma_wide", errs, tol)
    assert any(not errs[k] <= tol[k] for k in errs), errs
    assert not errs["align"] <= tol["align"]


@pytest.mark.parametrize("B,Tv", S.ENCODER_SHAPES)
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_encoder_cases_reach_exactly_one_and_are_well_conditioned(B, Tv, masked):
    hp, w, tokens, tl, ref, floor, ones, zeros = S.encoder_case(B, Tv, masked)
    print("encoder", B, Tv, masked, "floor %.3g  |h| == 1.0f share %.3g  |h| < 1e-6 share %.3g" % (floor, ones, zeros))
    assert S.FLOOR_FACTOR * floor <= S.ADMIT and ones > 0 and zeros > 0.05
    if masked:
        assert {1, 2, Tv} <= set(tl.tolist())
        for b, n in enumerate(tl):
            assert not ref[b, n:].any()
    hp0, w0 = S.recipe_weights("encoder", identity=True)
    f32 = oracle_np.encoder(hp0, oracle_np.cast_weights(w0, np.float32), tokens, np.float32, tl)
    assert not (np.abs(f32) == np.float32(1.0)).any()          # (Glorot scale: no state of exactly one)


def test_vocoder_case_is_saturated_and_well_conditioned():
    hp, w, mel, ref, floor, shares = S.vocoder_case()
    print("vocoder floor %.3g, float64 oracle's shares %s" % (floor, shares))
    assert ref.shape == S.VOCODER_SHAPE + (513,) and np.isfinite(ref).all()
    assert S.FLOOR_FACTOR * floor <= S.ADMIT
    assert all(shares[k] >= least for k, least in S.VOCODER_CONDITIONS), shares
    plain = S.vocoder_case(identity=True)[5]                   # (Glorot scale: no highway or BiLSTM gate beyond 8)
    assert plain["t_gt_8"] == 0 and plain["z_gt_8"] == 0, plain
    assert np.array_equal(ref, oracle_np.vocoder_taco1(hp, oracle_np.cast_weights(w, np.float64), mel.astype(np.float64), np.float64))
