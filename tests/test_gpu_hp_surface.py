"""GPU: encoder, postnet and CBHG vocoder off the shipped sizes (tests/hp_surface_cases.py) against the float64 oracle, each case on a
small context of its own (max_batch = B, max_tokens = Tv).  Every test asserts the launch forms its case is meant to reach -- the
dispatcher ids of gsttaco_encoder_variants / gsttaco_postnet_variants / gsttaco_vocoder_variants, the persistent-BiLSTM counter --
and prints its error and scale.  fp32 bound: max(TOL, 8 x the oracle's float32 floor) = TOL for every case (admitted on the CPU by
tests/test_hp_surface_cases.py); mixed precision: min(MIXED_TOL, drift / 2) against the bf16-emulating oracle."""
import gc

import numpy as np
import pytest

import hp_surface_cases as H
from gst_tacotron_amd import capi
from oracle import oracle_np
from test_gpu_parity import _assert_persistent_decode, _model, _sole_context

pytestmark = pytest.mark.gpu

V, VH = capi.CONV_V, capi.CONV_VH
IG = {v for k, v in V.items() if k.startswith("IG_")}                              # the fp32 implicit GEMM
BF16 = {v for k, v in V.items() if k.startswith(("C5_", "BF16_"))}                 # what a layer with a bf16 copy runs (mixed precision)
WINO_S = {V["WINO4_S"], V["WINO2_S"], V["WINO4_S_X3"], V["WINO2_S_X3"]}            # split Winograd, not bounded
WINO_ANY = WINO_S | {V["WINO4"], V["WINO2"]} | set(VH.values())
KNOBS = ("GSTTACO_BILSTM_PERSIST", "GSTTACO_LEAN", "GSTTACO_ENC_WINO", "GSTTACO_WINO", "GSTTACO_WINO_SPLIT", "GSTTACO_GRAPH",
         "GSTTACO_PERSIST_DECODE", "GSTTACO_FUSED_FRONT", "GSTTACO_PAD_DECODER")

ENCODER = [c.name for c in H.CASES if c.module == "encoder"]
POSTNET = [c.name for c in H.CASES if c.module == "postnet"]
VOCODER = [c.name for c in H.CASES if c.module == "vocoder"]


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _names(ids):
    return [capi.CONV_V_NAMES.get(v, v) for v in ids]


def _context(monkeypatch, name, B, Tv, env=None, mixed=False):
    """A context of the case's model under ``env`` (the library reads its knobs once, at create)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    _sole_context()
    hp, w = H.model_of(name, mixed)
    return _model(hp, w, B, Tv, 2)


def _check(what, got, ref, tol, scale=None):
    e = H.err(got, ref)
    print("%s: max abs err %.3g  tolerance %.3g  scale %.3g" % (what, e, tol, float(np.abs(ref).max()) if scale is None else scale))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    assert e <= tol, (what, e, tol)
    return e


def _assert_conv_forms(name, ids, want, mixed=False):
    """``want``: "ig" (an implicit-GEMM id on every layer; under mixed precision a bf16 id), or one of "ig" / "wino" / "wino_h" per layer."""
    want = [want] * len(ids) if isinstance(want, str) else list(want)
    assert len(want) == len(ids), (name, _names(ids), want)
    for i, (v, f) in enumerate(zip(ids, want)):
        ok = {"ig": BF16 if mixed else IG, "wino": WINO_S, "wino_h": {VH["WINO4_S"]}}[f]
        assert v in ok, (name, "layer", i, "runs", capi.CONV_V_NAMES.get(v, v), "not", f, _names(ids))


def _encode(m, name, shape, masked, slabs):
    """One m.encode of the case's tokens; the persistent-BiLSTM counter must advance by ``slabs`` on this first call of the shape."""
    tl = H.lengths_of(name, shape) if masked else None
    before = m.debug_counters()[0]
    got = _np(m.encode(H.inputs(name, shape), tl))
    m.synchronize()
    assert m.handoff_error() == 0
    assert m.debug_counters()[0] - before == slabs, (name, shape, "persistent BiLSTM launches", m.debug_counters()[0] - before, "expected", slabs)
    if masked:
        for b, n in enumerate(tl):
            assert not got[b, n:].any()
    return got


# ---------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("name", ENCODER)
def test_encoder_matches_the_oracle_and_takes_its_forms(monkeypatch, name):
    c = H.BY_NAME[name]
    for shape in c.shapes:
        B, Tv = shape
        m = _context(monkeypatch, name, B, Tv)
        ids, rows = m.encoder_variants(B, Tv)
        print(name, shape, "encoder layers run", _names(ids), "embedding rows launch:", rows)
        _assert_conv_forms(name, ids, c.forms["conv"])
        assert rows is c.forms["rows_path"]
        slabs = c.forms["persist"][shape]
        r = H.reference(name, shape)
        got = _encode(m, name, shape, False, slabs)
        _check("%s %s fp32" % (name, shape), got, r.ref, H.tolerance(r.floor))
        if c.lengths and shape in c.lengths:
            rm = H.reference(name, shape, True)
            _check("%s %s masked" % (name, shape), _encode(m, name, shape, True, slabs), rm.ref, H.tolerance(rm.floor))
        del m
        if slabs:
            # H == 256: the lean per-step form is the persistent launch's arithmetic, the general skinny form is not
            m = _context(monkeypatch, name, B, Tv, {"GSTTACO_BILSTM_PERSIST": "0"})
            lean = _encode(m, name, shape, False, 0)
            assert np.array_equal(lean, got), (name, shape, "lean per-step form differs from the persistent launch by", H.err(lean, got))
            del m
            m = _context(monkeypatch, name, B, Tv, {"GSTTACO_LEAN": "0"})
            _check("%s %s GSTTACO_LEAN=0" % (name, shape), _encode(m, name, shape, False, 0), r.ref, H.tolerance(r.floor))
            del m
        gc.collect()


def test_encoder_wino_case_without_the_winograd_gate(monkeypatch):
    """enc_wino_odd under GSTTACO_ENC_WINO=0: the same model as implicit GEMMs behind the token gather."""
    name, shape = "enc_wino_odd", (32, 420)
    m = _context(monkeypatch, name, *shape, env={"GSTTACO_ENC_WINO": "0"})
    ids, rows = m.encoder_variants(*shape)
    print(name, "GSTTACO_ENC_WINO=0: encoder layers run", _names(ids), "embedding rows launch:", rows)
    _assert_conv_forms(name, ids, "ig")
    assert rows is False
    r = H.reference(name, shape)
    _check("%s %s GSTTACO_ENC_WINO=0" % (name, shape), _encode(m, name, shape, False, 0), r.ref, H.tolerance(r.floor))
    rm = H.reference(name, shape, True)
    _check("%s %s GSTTACO_ENC_WINO=0 masked" % (name, shape), _encode(m, name, shape, True, 0), rm.ref, H.tolerance(rm.floor))


# ---------------------------------------------------------------------------------------------------- postnet
@pytest.mark.parametrize("name", POSTNET)
def test_postnet_matches_the_oracle_and_takes_its_forms(monkeypatch, name):
    c = H.BY_NAME[name]
    B = max(s[0] for s in c.shapes)
    m = _context(monkeypatch, name, B, 8)
    for shape in c.shapes:
        ids = m.postnet_variants(*shape)
        print(name, shape, "postnet layers run", _names(ids))
        assert len(ids) == len(m.dims.post_filters)
        _assert_conv_forms(name, ids, c.forms["conv"])
        r = H.reference(name, shape)
        _check("%s %s fp32" % (name, shape), _np(m.postnet(H.inputs(name, shape))), r.ref, H.tolerance(r.floor))


@pytest.mark.parametrize("knob", ["6", "0"])
def test_postnet_wino_case_on_the_other_winograd_forms(monkeypatch, knob):
    """post_wino_small under GSTTACO_WINO_SPLIT=6 (split-bf16 x6 on every layer, none bounded) and =0 (the fp32 Winograd kernel)."""
    name, shape = "post_wino_small", (32, 1920)
    m = _context(monkeypatch, name, shape[0], 8, env={"GSTTACO_WINO_SPLIT": knob})
    ids = m.postnet_variants(*shape)
    print(name, "GSTTACO_WINO_SPLIT=" + knob, "postnet layers run", _names(ids))
    assert set(ids) <= (WINO_S if knob == "6" else {V["WINO4"], V["WINO2"]}), _names(ids)
    r = H.reference(name, shape)
    _check("%s %s GSTTACO_WINO_SPLIT=%s" % (name, shape, knob), _np(m.postnet(H.inputs(name, shape))), r.ref, H.tolerance(r.floor))


# ---------------------------------------------------------------------------------------------------- vocoder
def _assert_vocoder_forms(m, name, shape, mixed=False):
    """enqueue_vocoder's stated rule: FP32, BF16 under mixed precision, never Winograd -- on every GEMM the model has."""
    forms = m.vocoder_variants(*shape)
    print(name, shape, "vocoder GEMMs run", {k: _names(v) for k, v in forms.items()})
    d = m.dims
    has = H.model_of(name)[1]
    assert {k: len(v) for k, v in forms.items()} == {
        "bank": d.bank_count, "proj": len(d.voc_proj_filters), "proj_dense": int("vocoder.proj_dense.kernel" in has),
        "highway_in": int("vocoder.highway_in.kernel" in has), "highway": d.highway_count, "dense": 1}
    for kind, ids in forms.items():
        for v in ids:
            assert v in (BF16 if mixed else IG) and v not in WINO_ANY, (name, kind, _names(ids))


@pytest.mark.parametrize("name", VOCODER)
def test_vocoder_matches_the_oracle_and_takes_its_forms(monkeypatch, name):
    c = H.BY_NAME[name]
    for shape in c.shapes:
        B, Tf = shape
        m = _context(monkeypatch, name, B, 8)
        _assert_vocoder_forms(m, name, shape)
        slabs = c.forms["persist"][shape]
        before = m.debug_counters()[0]
        r = H.reference(name, shape)
        got = _np(m.vocoder(H.inputs(name, shape)))
        m.synchronize()
        assert m.handoff_error() == 0 and m.debug_counters()[0] - before == slabs, (name, m.debug_counters(), slabs)
        assert got.shape == (B, Tf, m.dims.spec)
        _check("%s %s fp32" % (name, shape), got, r.ref, H.tolerance(r.floor))
        del m
        if slabs:
            m = _context(monkeypatch, name, B, 8, {"GSTTACO_BILSTM_PERSIST": "0"})
            lean = _np(m.vocoder(H.inputs(name, shape)))
            assert m.debug_counters()[0] == 0 and np.array_equal(lean, got), (name, H.err(lean, got))
            del m
            m = _context(monkeypatch, name, B, 8, {"GSTTACO_LEAN": "0"})
            _check("%s %s GSTTACO_LEAN=0" % (name, shape), _np(m.vocoder(H.inputs(name, shape))), r.ref, H.tolerance(r.floor))
            assert m.debug_counters()[0] == 0
            del m
        gc.collect()


# ---------------------------------------------------------------------------------------------------- mixed precision
@pytest.mark.parametrize("name", [c.name for c in H.CASES if c.mixed])
def test_mixed_precision_matches_the_bf16_emulating_oracle(monkeypatch, name):
    """Use_Mixed_Precision against the oracle that rounds the GEMM operands to bf16, at min(MIXED_TOL, drift / 2): a path that rounds no
    operand, or the wrong one, sits at about ``drift``.  The same model with the flag off is still the fp32 path."""
    c = H.BY_NAME[name]
    for shape in c.shapes:
        B, T = shape
        mr, r = H.mixed_reference(name, shape), H.reference(name, shape)
        tol = H.mixed_tolerance(mr.drift)
        results = {}
        for mixed in (True, False):
            m = _context(monkeypatch, name, B, T if c.module == "encoder" else 8, mixed=mixed)
            x = H.inputs(name, shape)
            if c.module == "encoder":
                ids, rows = m.encoder_variants(B, T)
                _assert_conv_forms(name, ids, "ig", mixed)
                before = m.debug_counters()[0]
                got = _np(m.encode(x))
                # (under bf16 the lean form exists only as the persistent launch: lean_bilstm_usable)
                assert m.debug_counters()[0] - before == c.forms["persist"][shape]
            elif c.module == "postnet":
                ids = m.postnet_variants(B, T)
                _assert_conv_forms(name, ids, "ig", mixed)
                got = _np(m.postnet(x))
            else:
                _assert_vocoder_forms(m, name, shape, mixed)
                before = m.debug_counters()[0]
                got = _np(m.vocoder(x))
                assert m.debug_counters()[0] - before == c.forms["persist"][shape]
            m.synchronize()
            assert m.handoff_error() == 0
            results[mixed] = got
            del m
        print("%s %s: drift %.3g, the emulation's own spread %.3g" % (name, shape, mr.drift, mr.spread))
        _check("%s %s mixed against the emulating oracle" % (name, shape), results[True], mr.ref, tol)
        _check("%s %s the flag off" % (name, shape), results[False], r.ref, H.tolerance(r.floor))
        gc.collect()


# ---------------------------------------------------------------------------------------------------- end to end
def _inference(m, c):
    out = m.Inference_Step(c.tokens, None, None, c.mels, c.mel_lengths, prenet_masks=c.masks, attn_noise=c.noise, steps=c.steps,
                           with_vocoder=True, return_pre_mel=True)
    m.synchronize()
    mel, stop, spec, align, pre = (_np(t) for t in out)
    return dict(zip(H.E2E_OUTPUTS, (mel, stop, spec, align, pre)))


@pytest.mark.parametrize("name", list(H.E2E))
def test_inference_step_end_to_end(monkeypatch, name):
    """Inference_Step(with_vocoder=True, return_pre_mel=True) with injected masks and noise, 8 steps, against oracle_np.inference_step.
    The tiny decoder is zero-padded onto the persistent decode launch (csrc/gsttaco.cpp pad_decoder): the test says which path ran."""
    c = H.e2e_case(name)
    ref, floor = H.e2e_reference(name)
    B, Tv = c.tokens.shape
    runs = {}
    for graph in (("1", "0") if name == "e2e_odd_gst" else ("1",)):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("GSTTACO_GRAPH", graph)
        _sole_context()
        m = _model(c.hp, c.w, B, Tv, c.mels.shape[1] if c.mels is not None else 2)
        runs[graph] = _inference(m, c)
        plan, counters = m.decode_plan(Tv), m.decode_counters()
        print("%s GSTTACO_GRAPH=%s: decode_plan (fused_front, fused_prenet0, lean) %s, persistent decode (launches, still on) %s,"
              " persistent BiLSTM %s" % (name, graph, plan, counters, m.debug_counters()))
        _assert_persistent_decode(m)
        assert m.handoff_error() == 0
        del m
        gc.collect()
    bad = []
    for k in H.E2E_OUTPUTS:
        g, r = runs["1"][k], ref[k]
        e, tol = H.err(g, r), H.tolerance(floor[k])
        print("%s %s: max abs err %.3g  floor %.3g  tolerance %.3g  scale %.3g" % (name, k, e, floor[k], tol, np.abs(r).max()))
        if not (g.shape == r.shape and np.isfinite(g).all() and e <= tol):
            bad.append((k, e, tol))
    assert not bad, bad
    if "0" in runs:
        for k in H.E2E_OUTPUTS:
            assert np.array_equal(runs["1"][k], runs["0"][k]), (name, k, "graph against eager", H.err(runs["1"][k], runs["0"][k]))
