"""GPU tests in the regime a trained model lives in (tests/saturated_cases.py: gates pinned at 0 and 1, a one-hot alignment that walks,
p that rounds to exactly 1.0f, tanh arguments in the tens, encoder states of exactly +-1.0f): the decode front ends and launch forms,
the persistent encoder BiLSTM, the vocoder's highway and BiLSTM and one whole Inference_Step against the float64 oracle, at cfg2
sizes, with injected masks and noise, graphs on.  Every case is admitted by the oracle alone first; the tolerance of an output is
max(TOL, 8 x its float32 floor), the floor from the oracle and never from a kernel."""
import gc

import numpy as np
import pytest

import saturated_cases as S
from oracle import oracle_np
from test_gpu_parity import _assert_persistent_decode, _model, _sole_context

pytestmark = pytest.mark.gpu

PATHS = {
    "persistent": {},                                                                   # persist_decode.hip: the default at <= 128 rows
    "launch": {"GSTTACO_PERSIST_DECODE": "0"},                                          # front_lean.h + fused LSTM + projection per step
    "four_kernel": {"GSTTACO_FUSED_FRONT": "0", "GSTTACO_PERSIST_DECODE": "0"},         # attention.hip
    "general_front": {"GSTTACO_FUSED_FRONT": "1", "GSTTACO_PERSIST_DECODE": "0"},       # front_body.h: the general fused kernel every step
    # (GSTTACO_LEAN=0 leaves the front end on front_lean.h; it moves the LSTM input halves and the projection to the general skinny GEMM bodies)
    "general": {"GSTTACO_LEAN": "0", "GSTTACO_PERSIST_DECODE": "0"},
}
KNOBS = ("GSTTACO_PERSIST_DECODE", "GSTTACO_FUSED_FRONT", "GSTTACO_LEAN", "GSTTACO_BILSTM_PERSIST")
DECODE = [
    ("sma_sharp", ("persistent", "launch", "four_kernel", "general_front", "general")),
    ("sma_sharp_group", ("persistent", "launch")),
    ("sma_wide", ("persistent", "launch", "four_kernel")),
    ("sma_long_masked", ("persistent", "launch")),
    ("bma", ("persistent", "launch", "four_kernel", "general_front", "general")),
    ("lsa_sharp", ("persistent", "launch", "four_kernel")),
    ("lsa_smooth", ("persistent", "launch", "four_kernel")),
]


def _np(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _setenv(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _decode_on(monkeypatch, c, enc, gst, path):
    """One model under the path's knobs, the case decoded twice from the oracle's memory (the second call replays the captured graph)."""
    _setenv(monkeypatch, PATHS[path])
    _sole_context()
    m = _model(c.hp, c.w, c.spec.B, c.spec.Tv, 2)
    outs = [_np(*m.decode(enc, gst, c.masks, c.noise, steps=c.spec.steps, token_lengths=c.token_lengths)) for _ in range(2)]
    m.synchronize()
    assert m.handoff_error() == 0
    if path == "persistent":
        _assert_persistent_decode(m)
    else:
        assert m.decode_counters() == (0, 0)
    if path == "four_kernel":
        assert m.decode_plan(c.spec.Tv)[0] is False
    if path == "general_front":
        assert m.decode_plan(c.spec.Tv)[0] is True
    if path == "general":
        assert m.decode_plan(c.spec.Tv)[2] is False
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    del m
    gc.collect()
    return outs[0]


@pytest.mark.parametrize("name,paths", DECODE, ids=[d[0] for d in DECODE])
def test_saturated_decode_matches_the_oracle_on_every_path(monkeypatch, name, paths):
    c, m = S.measured(name)
    print(S.describe(name, m))
    assert S.admit(m, S.CONDITIONS[name], ("pre_mel", "stop", "align")) == []
    enc, gst = m["ref"]["encoder"].astype(np.float32), m["ref"]["gst"].astype(np.float32)
    keys = ("pre_mel", "stop", "align")
    tol = {k: S.tolerance(m["floor"][k]) for k in keys}
    got, bad = {}, []
    for path in paths:
        got[path] = _decode_on(monkeypatch, c, enc, gst, path)
        errs = {k: S._err(g, m["ref"][k]) for k, g in zip(keys, got[path])}
        print("%s %s: max abs err vs the float64 oracle %s  tolerance %s" % (name, path, errs, tol))
        for k, g in zip(keys, got[path]):
            assert g.shape == m["ref"][k].shape
            if not (np.isfinite(g).all() and errs[k] <= tol[k]):
                bad.append((path, k, errs[k], tol[k]))
    assert not bad, bad
    if c.token_lengths is not None:
        for b, n in enumerate(c.token_lengths):
            assert not got["persistent"][2][b][:, n:].any()
    # the persistent launch and the launch path are the same arithmetic in the same order HERE too: a clamp that one caller puts around
    # the shared BMA / SMA / softmax chain shows up as a difference first
    for k, a, b in zip(keys, got["persistent"], got["launch"]):
        assert np.array_equal(a, b), (name, k, float(np.abs(a - b).max()))
    # the launch path's lean front kernel and the general front kernel call the same chain functions behind heads that sum alike
    if "general_front" in got:
        for k, a, b in zip(keys, got["launch"], got["general_front"]):
            assert np.array_equal(a, b), (name, k, float(np.abs(a - b).max()))


def test_saturated_mixed_precision_persistent_is_bitwise_the_launch_path(monkeypatch):
    """The bf16 persistent kernel against the bf16 launch path on SMA sharp at 40 x 40: bitwise, finite.  (Not against the oracle: under
    bf16 operands a saturated recurrence amplifies a flipped rounding, which is no statement about a kernel.)"""
    c = S.make_case("sma_sharp_mixed")
    assert c.hp["Use_Mixed_Precision"] is True
    w64 = oracle_np.cast_weights(c.w, np.float64)
    enc = oracle_np.encoder(c.hp, w64, c.tokens, np.float64).astype(np.float32)
    gst = oracle_np.style_token_layer(c.hp, w64, c.mels, c.mel_lengths, np.float64).astype(np.float32)
    got = {path: _decode_on(monkeypatch, c, enc, gst, path) for path in ("persistent", "launch")}
    for a, b in zip(got["persistent"], got["launch"]):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    assert got["persistent"][2].max() > 0.9                                  # (the alignment is sharp in this mode too)


@pytest.mark.parametrize("B,Tv", S.ENCODER_SHAPES)
def test_saturated_encoder_bilstm_persistent_is_bitwise_the_per_step_form(monkeypatch, B, Tv):
    """States of exactly +-1.0f and of (nearly) 0 through the persistent BiLSTM, whose hand-off tag lives in bit 30 of the state word
    (|h| < 2): bitwise the per-step kernel, both within tolerance of the float64 oracle, unmasked and masked (lengths 1, 2 and full),
    two calls on the same model so the tags are re-used."""
    enc = {}
    for knob in ("1", "0"):
        _setenv(monkeypatch, {"GSTTACO_BILSTM_PERSIST": knob})
        _sole_context()
        hp, w = S.recipe_weights("encoder")
        m = _model(hp, w, B, Tv, 2)
        assert m.debug_counters()[1] == int(knob)
        for masked in (False, True):
            hp, w, tokens, tl, ref, floor, ones, zeros = S.encoder_case(B, Tv, masked)
            assert S.FLOOR_FACTOR * floor <= S.ADMIT and ones > 0
            for rep in range(2):
                got = _np(m.encode(tokens, tl))[0]
                err = S._err(got, ref)
                print("encoder %d x %d %s knob %s call %d: err %.3g floor %.3g tolerance %.3g  |h| == 1.0f share: oracle %.3g kernel %.3g"
                      % (B, Tv, "masked" if masked else "unmasked", knob, rep, err, floor, S.tolerance(floor), ones,
                         (np.abs(got) == np.float32(1.0)).mean()))
                assert np.isfinite(got).all() and err <= S.tolerance(floor)
                if masked:
                    for b, n in enumerate(tl):
                        assert not got[b, n:].any()
                enc[(knob, masked, rep)] = got
        m.synchronize()
        assert m.handoff_error() == 0
        n, on = m.debug_counters()
        assert (n >= 2 and on == 1) if knob == "1" else (n == 0 and on == 0)
        del m
        gc.collect()
    for key, v in enc.items():
        if key[0] == "1":
            assert np.array_equal(v, enc[("0",) + key[1:]]), key
            assert np.array_equal(v, enc[("1", key[1], 0)])


def test_saturated_vocoder_matches_the_oracle():
    """Highway gates of 1 / (1 + expf(-t)) with |t| beyond 8 and a BiLSTM with gates beyond 16, 3 x 21 frames."""
    hp, w, mel, ref, floor, shares = S.vocoder_case()
    assert S.FLOOR_FACTOR * floor <= S.ADMIT and all(shares[k] >= least for k, least in S.VOCODER_CONDITIONS), shares
    m = _model(hp, w, S.VOCODER_SHAPE[0], 8, 2)
    spec = _np(m.vocoder(mel))[0]
    err = S._err(spec, ref)
    print("vocoder: err %.3g floor %.3g tolerance %.3g scale %.3g shares %s" % (err, floor, S.tolerance(floor), np.abs(ref).max(), shares))
    assert spec.shape == ref.shape and np.isfinite(spec).all() and err <= S.tolerance(floor)
    assert m.handoff_error() == 0


def test_saturated_inference_step_end_to_end_with_vocoder():
    """One whole Inference_Step(with_vocoder=True) on SMA sharp, 5 x 40 over 8 steps, against oracle_np.inference_step (held equal to
    the helper's reference on the CPU); the device's own report sees no non-finite value on any row."""
    c, m = S.measured("sma_sharp")
    outputs = ("encoder", "e2e_mel", "e2e_stop", "e2e_align", "e2e_spectrogram")
    assert S.admit(m, S.CONDITIONS["sma_sharp"], outputs) == []
    _sole_context()
    model = _model(c.hp, c.w, c.spec.B, c.spec.Tv, c.mels.shape[1])
    out = model.Inference_Step(c.tokens, None, None, c.mels, c.mel_lengths, prenet_masks=c.masks, attn_noise=c.noise, steps=c.spec.steps,
                               with_vocoder=True)
    model.synchronize()
    _assert_persistent_decode(model)
    report, _ = model.Utterance_Report(out[1], out[3], None, out[0])
    mel, stop, spec, align, report = _np(*out, report)
    ref = oracle_np.inference_step(c.hp, c.w, c.tokens, c.mels, c.mel_lengths, c.masks, c.noise, steps=c.spec.steps, dt=np.float64,
                                   with_vocoder=True)
    bad = []
    for k, g, r in (("e2e_mel", mel, ref[0]), ("e2e_stop", stop, ref[1]), ("e2e_spectrogram", spec, ref[2]), ("e2e_align", align, ref[3])):
        err, tol = S._err(g, r), S.tolerance(m["floor"][k])
        print("end to end %s: err %.3g floor %.3g tolerance %.3g" % (k, err, m["floor"][k], tol))
        if not (g.shape == r.shape and np.isfinite(g).all() and err <= tol):
            bad.append((k, err, tol))
    assert not bad, bad
    from gst_tacotron_amd.model import REPORT_FIELDS
    assert report.shape == (c.spec.B, len(REPORT_FIELDS)) and not report[:, REPORT_FIELDS.index("nonfinite")].any()
    assert model.handoff_error() == 0
