"""CPU: the float64 reference of the conv/GEMM dispatcher (oracle/conv_ref.py) against plain loops and the model oracle, and the
dispatcher's variant list (include/gsttaco.h GSTTACO_CONV_V_* / GSTTACO_CONV_FORM_*) against capi.py's mirror."""
import os
import re

import numpy as np
import pytest

from gst_tacotron_amd import capi
from oracle import conv_ref, oracle_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_enum(prefix):
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b" + prefix + r"([A-Z0-9_]+)\s*=\s*(-?\d+)", header)}


def test_header_conv_variants_match_capi():
    hv = _header_enum("GSTTACO_CONV_V_")
    assert hv.pop("INVALID") == capi.CONV_V_INVALID
    assert hv.pop("COUNT") == len(capi.CONV_V)
    assert hv == capi.CONV_V
    assert sorted(hv.values()) == list(range(len(hv)))          # dense: a coverage test can ask for every one of them
    assert _header_enum("GSTTACO_CONV_FORM_") == capi.CONV_FORM


def _case(rng, B, T, Cin, N, taps, vocab=None):
    x = rng.standard_normal(((vocab or B * T), Cin))
    w = rng.standard_normal((taps * Cin, N))
    return x, w


@pytest.mark.parametrize("taps,pad_before", [(1, 0), (3, 1), (4, 1), (4, 2), (5, 2), (2, 0), (5, 4)])
@pytest.mark.parametrize("flags", ["plain", "tokens", "row_len", "pool2", "epilogue_relu", "epilogue_tanh"])
def test_reference_matches_naive_loops(taps, pad_before, flags):
    rng = np.random.default_rng(taps * 10 + pad_before)
    B, T, Cin, N, vocab = 3, 7, 4, 5, 9
    tokens = rng.integers(0, vocab, (B, T)) if flags == "tokens" else None
    if tokens is not None:
        tokens[0, 0], tokens[-1, -1] = 0, vocab - 1
    x, w = _case(rng, B, T, Cin, N, taps, vocab if tokens is not None else None)
    kw = dict(pad_before=pad_before, tokens=tokens)
    if flags in ("row_len", "pool2", "epilogue_relu"):
        kw["row_len"] = np.array([0, 4, T + 3])
    if flags == "pool2":
        kw["pool2"] = True
    if flags.startswith("epilogue"):
        kw.update(scale=rng.standard_normal(N), shift=rng.standard_normal(N), rowbias=rng.standard_normal((B, N)),
                  res=rng.standard_normal((B * T, N)), act=conv_ref.ACT_RELU if flags == "epilogue_relu" else conv_ref.ACT_TANH)
    y, m = conv_ref.conv_gemm_ref(x, w, B, T, Cin, N, taps, **kw)
    y0 = conv_ref.conv_gemm_naive(x, w, B, T, Cin, N, taps, **kw)
    np.testing.assert_allclose(y, y0, rtol=1e-12, atol=1e-12)
    # the magnitude is the same contract on absolute values (before act / res)
    kabs = dict(kw)
    for k in ("act", "res"):
        kabs.pop(k, None)
    for k in ("scale", "shift", "rowbias"):
        if k in kabs:
            kabs[k] = np.abs(kabs[k])
    if not kw.get("pool2"):       # (max of absolute values is not the absolute value of the max: compare the plain gather only)
        m0 = conv_ref.conv_gemm_naive(np.abs(x), np.abs(w), B, T, Cin, N, taps, **kabs)
        np.testing.assert_allclose(m, m0, rtol=1e-12, atol=1e-12)
    assert np.all(m >= 0)


def test_reference_ldw_ignores_columns_past_n():
    rng = np.random.default_rng(1)
    B, T, Cin, N, taps = 2, 5, 4, 5, 3
    x, w = _case(rng, B, T, Cin, N, taps)
    wp = np.concatenate([w, np.full((taps * Cin, 3), np.nan)], 1)
    y, _ = conv_ref.conv_gemm_ref(x, wp, B, T, Cin, N, taps, pad_before=1, ldw=N + 3)
    y0, _ = conv_ref.conv_gemm_ref(x, w, B, T, Cin, N, taps, pad_before=1)
    np.testing.assert_array_equal(y, y0)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
def test_reference_matches_oracle_conv1d_same(k):
    rng = np.random.default_rng(k)
    B, T, Cin, N = 2, 11, 6, 4
    x = rng.standard_normal((B, T, Cin))
    kern = rng.standard_normal((k, Cin, N))
    _, pb, _ = oracle_np.same_pad(T, k, 1)
    y, _ = conv_ref.conv_gemm_ref(x, kern.reshape(k * Cin, N), B, T, Cin, N, k, pad_before=pb)
    np.testing.assert_allclose(y.reshape(B, T, N), oracle_np.conv1d_same(x, kern), rtol=1e-12, atol=1e-12)


def test_reference_pool2_matches_oracle_maxpool():
    rng = np.random.default_rng(2)
    B, T, Cin, N, k = 2, 9, 4, 3, 3
    x = rng.standard_normal((B, T, Cin))
    kern = rng.standard_normal((k, Cin, N))
    y, _ = conv_ref.conv_gemm_ref(x, kern.reshape(k * Cin, N), B, T, Cin, N, k, pad_before=1, pool2=True)
    np.testing.assert_allclose(y.reshape(B, T, N), oracle_np.conv1d_same(oracle_np.maxpool1d_same2(x), kern), rtol=1e-12, atol=1e-12)
    # padding never wins the max: all-negative input, the last frame is itself
    xn = -np.abs(x) - 1.0
    y, _ = conv_ref.conv_gemm_ref(xn, np.eye(Cin), B, T, Cin, Cin, 1, pool2=True)
    np.testing.assert_array_equal(y.reshape(B, T, Cin)[:, -1], xn[:, -1])


@pytest.mark.parametrize("H,W,k,stride", [(9, 7, 3, 2), (8, 8, 3, 2), (5, 6, 3, 1), (7, 5, 2, 2)])
def test_reference_conv2d_matches_oracle(H, W, k, stride):
    rng = np.random.default_rng(H * W)
    B, Cin, N = 2, 4, 5
    x = rng.standard_normal((B, H, W, Cin))
    kern = rng.standard_normal((k, k, Cin, N))
    Ho, ph, _ = oracle_np.same_pad(H, k, stride)
    Wo, pw, _ = oracle_np.same_pad(W, k, stride)
    geo = dict(H=H, W=W, kh=k, kw=k, stride=stride, pad_h=ph, pad_w=pw, Wo=Wo)
    y, _ = conv_ref.conv_gemm_ref(x, kern.reshape(k * k * Cin, N), B, Ho * Wo, Cin, N, k * k, conv2d=geo)
    np.testing.assert_allclose(y.reshape(B, Ho, Wo, N), oracle_np.conv2d_same(x, kern, stride), rtol=1e-12, atol=1e-12)


def test_reference_bf16_rounds_both_operands():
    rng = np.random.default_rng(3)
    B, T, Cin, N = 1, 6, 8, 4
    x = rng.standard_normal((B * T, Cin))
    w = rng.standard_normal((Cin, N))
    y, _ = conv_ref.conv_gemm_ref(x, w, B, T, Cin, N, 1, bf16=True)
    r = lambda a: oracle_np.bf16_round(a.astype(np.float32)).astype(np.float64)      # noqa: E731
    np.testing.assert_allclose(y, r(x) @ r(w), rtol=1e-12, atol=1e-12)


def test_reference_rejects_tokens_with_pool2():
    with pytest.raises(ValueError):
        conv_ref.gather_rows(np.zeros((4, 4)), 1, 2, 4, 1, 0, tokens=np.zeros((1, 2), int), pool2=True)
