"""CPU: the cases of tests/test_gpu_style.py are well conditioned and can see what they are meant to see, and the host side of the
style-control extension (the binding's symbol list, the header, the Feeder) is in place.  No GPU involved."""
import os
import re

import numpy as np
import pytest

import gst_cases as G
import style_cases as S
from test_gpu_parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gsttaco_gst_ex", "gsttaco_style_compose", "gsttaco_inference_step_styled")


def _max(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("name", S.CASES)
def test_compose_of_the_exported_pair_is_the_embedding(name):
    """float64 compose(p, q) IS style_token_layer (the same sums in the same order: difference 0), and a float32 evaluation of it stays
    within TOL / 5 of the float64 one, so the GPU's float32 arithmetic has room under TOL."""
    hp, w, shape, mel = S.case(name)
    p, q = S.exported(name)
    H, N, A = S.dims(hp)
    assert p.shape == (shape.B, H, N) and q.shape == (shape.B, A) and shape.B == 3
    ref = S.reference(name)
    d64 = _max(S.compose(hp, w, p, q), ref)
    p32, q32 = S.export(hp, w, *G.inputs(shape, mel), dt=np.float32)
    d32 = _max(S.compose(hp, w, p32, q32, dt=np.float32), ref)
    print(name, "compose(p, q) against style_token_layer: float64", d64, "float32", d32)
    assert d64 <= 1e-14
    assert d32 <= TOL / 5


@pytest.mark.parametrize("name", S.CASES)
def test_signed_weights_are_well_conditioned(name):
    hp, w, _, _ = S.case(name)
    tw = S.signed_weights(name)
    assert tw.min() < 0.0 < tw.max() and tw.dtype == np.float32          # (signed; one head x one token has three numbers)
    err = _max(S.compose(hp, w, tw, dt=np.float32), S.signed_reference(name))
    print(name, "signed weights, no query: float32 against float64", err)
    assert np.isfinite(S.signed_reference(name)).all()
    assert err <= TOL / 5


@pytest.mark.parametrize("name", S.CASES + ["cfg2_short", "sharp_short"])
def test_exports_are_well_conditioned(name):
    hp, w, shape, mel = S.case(name)
    p, q = S.exported(name)
    p32, q32 = S.export(hp, w, *G.inputs(shape, mel), dt=np.float32)
    print(name, "float32 against float64: p", _max(p32, p), "q", _max(q32, q), "; largest weight", float(p.max()))
    assert np.abs(p.sum(-1) - 1.0).max() <= 1e-12
    assert _max(p32, p) <= TOL / 5
    assert _max(q32, q) <= TOL / 5


@pytest.mark.parametrize("name", [n for n in S.CASES if S.dims(S.case(n)[0])[0] > 1])
def test_compose_sees_heads_in_the_wrong_order(name):
    """Signed weights whose heads are rotated by one -- what a wrong head stride or slice gives -- move the result by at least
    100 x TOL (measured: >= 3.4 on every multi-head case)."""
    hp, w, _, _ = S.case(name)
    tw = S.signed_weights(name)
    moved = _max(S.compose(hp, w, np.roll(tw, 1, axis=1)), S.signed_reference(name))
    print(name, "heads rotated by one move the composed embedding by", moved)
    assert moved >= 100 * TOL


def test_zero_weights_give_beta():
    for name in S.CASES:
        hp, w, shape, _ = S.case(name)
        H, N, A = S.dims(hp)
        for dt in (np.float64, np.float32):
            got = S.compose(hp, w, np.zeros((shape.B, H, N), dt), dt=dt)
            assert np.array_equal(got, np.broadcast_to(w["gst.mha.ln.beta"].astype(dt), (shape.B, A))), name


def test_sharpened_weights_make_the_export_see_swapped_heads():
    """At the plain cfg2 weights the attention is nearly uniform: the largest weight of 16 tokens is 0.12, and a p with its heads
    rotated by one is at most 0.08 from the right one.  The query kernel scaled by 8 gives a largest weight of 0.65 and a gap between
    the right p and the rotated one of at least 0.38 on every utterance of G.SHORT (measured here, printed below): 76 x the required
    100 x TOL = 5e-3.  The grid case of the export test (8 heads x 33 tokens, largest weight 0.037) keeps 0.0097."""
    plain, _ = S.exported("cfg2_short")
    p, _ = S.exported("sharp_short")
    gap = np.abs(np.roll(p, 1, axis=1) - p).reshape(p.shape[0], -1).max(axis=1)
    plain_gap = np.abs(np.roll(plain, 1, axis=1) - plain).reshape(plain.shape[0], -1).max(axis=1)
    print("largest weight: plain", float(plain.max()), "sharpened", float(p.max()),
          "; heads rotated by one: plain gap", float(plain_gap.min()), "sharpened gap", float(gap.min()))
    assert p.max() > plain.max()
    assert gap.min() >= 100 * TOL
    # ... and the grid case of the export test, 8 heads x 33 tokens, sees it too
    pg, _ = S.exported("u64_dense64_att256_heads8_tok33")
    gg = np.abs(np.roll(pg, 1, axis=1) - pg).reshape(pg.shape[0], -1).max(axis=1)
    print("u64_dense64_att256_heads8_tok33: heads rotated by one gap", float(gg.min()))
    assert gg.min() >= 100 * TOL


def test_binding_and_header_carry_the_style_entry_points():
    from gst_tacotron_amd import capi
    assert capi.ABI_VERSION == 14
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    assert re.search(r"#define\s+GSTTACO_ABI_VERSION\s+14\b", header)
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name


def test_feeder_returns_tokens_alone_when_the_style_is_given(capsys):
    from gst_tacotron_amd import synthetic
    from gst_tacotron_amd.feeder import Feeder
    from gst_tacotron_amd.hparams import load_token_dict
    hp = synthetic.tiny_hp()
    assert hp["GST"]["Use"]
    f = Feeder(hp, load_token_dict(hp))
    sentences = ["Hello there.", "Hi."]
    pat = f.Get_Inference_Pattern(sentences, None, style_given=True)
    out = capsys.readouterr().out
    assert "no wav information" not in out
    assert pat is not None and set(pat) == {"tokens", "token_lengths", "initial_mels"}
    assert pat["tokens"].shape == (2, len(sentences[0]) + 2) and list(pat["token_lengths"]) == [len(s) + 2 for s in sentences]
    # the default is unchanged: the reference's message and None
    assert f.Get_Inference_Pattern(sentences, None) is None
    assert "GST is enabled, but no wav information." in capsys.readouterr().out
