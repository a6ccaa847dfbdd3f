"""GPU: the bounded-input form of the split Winograd kernel (conv_wino_split.hip, plane mode fp16 x3: two fp16 planes per operand,
products hh hl lh, the input transform scaled by 2^SV and every weight column by 2^SU[n]) against the float64 reference
(oracle/conv_ref.py), through gsttaco_debug_conv_prepare / _run like test_gpu_conv_kernels.py, whose bound and helpers it uses.

A call reaches the form only with the WINO_SPLIT_H planes AND a promised input bound (ConvCall.x_absmax <= 1); each case asserts the
variant it ran.  Shapes: the smallest at which the dispatcher picks each transform (240 workgroups), cin = 128 (four 32-channel slices:
the kernel's minimum) and one cin = 512.  Inputs per shape:
  tanh    tanh of N(0, 1.5): what a postnet layer behind a tanh reads
  sat     exactly +-1 everywhere, in the period-4 pattern + + - - along time that makes the F(4,5) transform's row of sum 15 (and the
          F(2,5) row of sum 3) reach its sum on EVERY tile and channel: |V 2^SV| = 30 720, the overflow edge
  tiny    |x| <= 2^-12: low planes at and below fp16's normal range, the flush edge; no scale / shift (the epilogue scale is then the
          power of two alone), so that the error is the GEMMs' own -- held to 1.6 x the absolute error of the fp32-pipe Winograd kernel
          (forms FP32 | WINO2 | WINO4) on the same data
Weights: Gaussian / sqrt(K), with column 0 all zero, column 1 scaled by 2^-20 and column 2 by 2^6.
Bound (tanh, sat): the module's Winograd bound C_WINO[MO] 2^-24 m + one epilogue rounding, m the largest magnitude over the tile.

Measured on the MI355X (units of 2^-24 m against C_WINO = 56; tiny: largest absolute error, this form / the fp32 pipe):
  F4_N512         tanh 4.22  sat 5.12  tiny 4.10e-08 / 6.06e-08
  F2_N512         tanh 6.63  sat 3.42  tiny 3.05e-08 / 4.96e-08
  F2_N80_res      tanh 5.30  sat 2.71  tiny 3.70e-08 / 4.98e-08
  F4_N80          tanh 7.12  sat 3.80  tiny 5.48e-08 / 7.50e-08
  F4_N512_cin512  tanh 7.85  sat 4.67  tiny 7.29e-08 / 1.41e-07
  postnet (8, 1024): 9.24e-06 with the form, 9.83e-06 with x6 everywhere (bar 5e-5)
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import test_gpu_conv_kernels as ck
from gst_tacotron_amd import capi
from oracle import conv_ref

pytestmark = pytest.mark.gpu

U = ck.U
F = capi.CONV_FORM
V, VH = capi.CONV_V, capi.CONV_VH
FORMS_H = ck.SPLIT_WINO | F["WINO_SPLIT_H"]
WINO_OF = {VH["WINO4_S"]: 4, VH["WINO2_S"]: 2, V["WINO4_S"]: 4, V["WINO2_S"]: 2, V["WINO4"]: 4, V["WINO2"]: 2}
X6_OF = {VH["WINO4_S"]: V["WINO4_S"], VH["WINO2_S"]: V["WINO2_S"]}
FP32_OF = {VH["WINO4_S"]: V["WINO4"], VH["WINO2_S"]: V["WINO2"]}


def case(name, expect, B, T, cin, n, act=0, res=False, row_len=None):
    return dict(name=name, expect=expect, B=B, T=T, cin=cin, n=n, act=act, res=res, row_len=row_len)


CASES = [
    case("F4_N512", VH["WINO4_S"], 3, 5033, 128, 512, act=2, row_len=[5033, 5000, 4]),
    case("F2_N512", VH["WINO2_S"], 3, 2517, 128, 512),
    case("F2_N80_res", VH["WINO2_S"], 4, 7650, 128, 80, res=True),          # a partial column block
    case("F4_N80", VH["WINO4_S"], 4, 15300, 128, 80),
    case("F4_N512_cin512", VH["WINO4_S"], 3, 5033, 512, 512),              # the slice loop at the postnet's length
]


def teardown_module(module):
    ck.teardown_module(module)


def test_case_table_reaches_both_bounded_variants():
    assert {c["expect"] for c in CASES} == set(VH.values())


def make_weights(c, rng):
    K, n = 5 * c["cin"], c["n"]
    w = rng.standard_normal((K, n)) / np.sqrt(K)
    w[:, 0] = 0.0
    w[:, 1] *= 2.0 ** -20
    w[:, 2] *= 2.0 ** 6
    return dict(w=ck.f32(w), scale=ck.f32(rng.uniform(0.5, 1.5, n) * rng.choice([-1, 1], n)), shift=ck.f32(rng.standard_normal(n)),
                res=ck.f32(rng.standard_normal((c["B"] * c["T"], n))) if c["res"] else None)


def make_x(c, kind, rng):
    B, T, cin = c["B"], c["T"], c["cin"]
    if kind == "tanh":
        return ck.f32(np.tanh(rng.normal(0, 1.5, (B * T, cin))))
    if kind == "sat":
        s = np.where((np.arange(T) % 4) % 3 == 0, 1.0, -1.0)            # t = 0, 3 (mod 4): +, t = 1, 2: -
        return (s[None, :, None] * rng.choice([-1.0, 1.0], (B, 1, cin))).reshape(B * T, cin)
    return ck.f32(rng.uniform(-1, 1, (B * T, cin)) * 2.0 ** -12)


def run(c, wid, forms, x, x_absmax, act, res, ldo=None):
    """One dispatcher call; returns (variant, out [M, N] float64).  Sentinel-filled output with guard rows and columns."""
    h = ck.hook(False)
    dev = torch.device("cuda")
    M, N = c["B"] * c["T"], c["n"]
    ldo = ldo or N + 4
    out = torch.full((M + ck.GUARD_ROWS, ldo), ck.SENTINEL, dtype=torch.float32, device=dev)
    t = lambda a, dt=torch.float32: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)   # noqa: E731
    resd = None
    if res is not None:
        resd = torch.zeros((M, ldo), dtype=torch.float32, device=dev)
        resd[:, :N] = t(res)
    call = capi.ConvCall()
    call.forms, call.B, call.T, call.pad_before, call.act, call.ldo = forms, c["B"], c["T"], 2, act, ldo
    call.x_absmax = x_absmax
    rl = None if c["row_len"] is None else t(np.asarray(c["row_len"], np.int32), torch.int32)
    v = h.run(wid, call, t(x), out, row_len=rl, res=resd)
    torch.cuda.synchronize()
    o = out.cpu().numpy().astype(np.float64)
    assert np.all(o[M:] == ck.SENTINEL), "{}: a guard row was written".format(c["name"])
    assert np.all(o[:M, N:] == ck.SENTINEL), "{}: a column in [N, ldo) was written".format(c["name"])
    return v, o[:M, :N]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_bounded_form_case(c):
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    h = ck.hook(False)
    d = make_weights(c, rng)
    n, cin = c["n"], c["cin"]
    wid = h.prepare(d["w"], 5, cin, n, n, FORMS_H, d["scale"], d["shift"])
    rl = None if c["row_len"] is None else np.asarray(c["row_len"], np.int32)
    mo = WINO_OF[c["expect"]]
    report = []
    for kind in ("tanh", "sat"):
        x = make_x(c, kind, rng)
        assert np.abs(x).max() <= 1.0
        act = c["act"] if kind == "tanh" else 0          # (saturated inputs behind a tanh epilogue would hide the GEMMs' error)
        v, y = run(c, wid, FORMS_H, x, 1.0, act, d["res"])
        assert v == c["expect"], (c["name"], kind, capi.CONV_V_NAMES.get(v, v))
        yr, m = conv_ref.conv_gemm_ref(x, d["w"], c["B"], c["T"], cin, n, 5, pad_before=2, row_len=rl, scale=d["scale"], shift=d["shift"],
                                       act=act, res=d["res"])
        mt = ck.tile_magnitude(dict(B=c["B"], T=c["T"]), m, mo)
        tol = ck.C_WINO[mo] * U * mt + 2 * U * np.abs(yr) + (ck.TANH_ABS if act == 2 else 0.0)
        assert np.all(np.isfinite(y)), (c["name"], kind)
        err = np.abs(y - yr)
        ratio = float(np.max((err - (tol - ck.C_WINO[mo] * U * mt)) / (U * np.maximum(mt, 1e-30))))
        report.append("{} {:.2f} units (C {})".format(kind, ratio, ck.C_WINO[mo]))
        print("\n{} {}: {:.2f} units of 2^-24 m".format(c["name"], kind, ratio))
        worst = np.unravel_index(np.argmax(err - tol), y.shape)
        assert np.all(err <= tol), "{} {}: {:.2f} units of 2^-24 m > C = {} at {}: {} vs {}".format(
            c["name"], kind, ratio, ck.C_WINO[mo], worst, y[worst], yr[worst])
        # the all-zero column carries the shift alone, whatever the planes hold
        if act == 0 and d["res"] is None:
            assert np.all(y[:, 0] == d["shift"][0])
    # tiny inputs: no scale / shift, against the fp32-pipe kernel's own absolute error on the same data
    wid0 = h.prepare(d["w"], 5, cin, n, n, FORMS_H, None, None)
    x = make_x(c, "tiny", rng)
    yr, _ = conv_ref.conv_gemm_ref(x, d["w"], c["B"], c["T"], cin, n, 5, pad_before=2, row_len=rl)
    v, y = run(c, wid0, FORMS_H, x, 1.0, 0, None)
    assert v == c["expect"]
    v32, y32 = run(c, wid0, ck.FP32_WINO, x, 0.0, 0, None)
    assert v32 == FP32_OF[c["expect"]], capi.CONV_V_NAMES.get(v32, v32)
    e_new, e_32 = float(np.abs(y - yr).max()), float(np.abs(y32 - yr).max())
    print("{} tiny: largest absolute error {:.3e} (fp32 pipe {:.3e}, ratio {:.2f})".format(c["name"], e_new, e_32, e_new / e_32))
    assert e_new <= 1.6 * e_32, "{} tiny: {:.3e} > 1.6 x {:.3e} (the fp32-pipe kernel on the same data)".format(c["name"], e_new, e_32)
    print("{:16s} {:10s} {}".format(c["name"], capi.CONV_V_NAMES[c["expect"]], "; ".join(report)))


def test_without_a_bound_or_without_the_planes_the_x6_form_runs():
    """The negative control: the same call with no promise, with a promise the form is not built for, or without the WINO_SPLIT_H bit
    reports -- and runs -- the split-bf16 x6 variant; with GSTTACO_WINO_SPLIT's reduced-form flag the x3 knob keeps its meaning."""
    for c in (CASES[0], CASES[2]):
        rng = np.random.default_rng(1)
        d = make_weights(c, rng)
        wid = ck.hook(False).prepare(d["w"], 5, c["cin"], c["n"], c["n"], FORMS_H, d["scale"], d["shift"])
        x = make_x(c, "tanh", rng)
        x6 = X6_OF[c["expect"]]
        vh, yh = run(c, wid, FORMS_H, x, 1.0, 0, d["res"])
        assert vh == c["expect"]
        ys = []
        for forms, bound in ((FORMS_H, 0.0), (FORMS_H, 2.0), (ck.SPLIT_WINO, 1.0), (ck.SPLIT_WINO, 0.0)):
            v, y = run(c, wid, forms, x, bound, 0, d["res"])
            assert v == x6, (c["name"], forms, bound, capi.CONV_V_NAMES.get(v, v))
            ys.append(y)
        assert all(np.array_equal(ys[0], y) for y in ys[1:])              # one kernel, one result
        assert not np.array_equal(ys[0], yh)                               # ... and not the fp16 form's
        # a bound below 1 is a promise too
        v, y = run(c, wid, FORMS_H, x, 0.999, 0, d["res"])
        assert v == c["expect"] and np.array_equal(y, yh)


def test_postnet_takes_the_bounded_form_behind_tanh_only(monkeypatch):
    """The whole postnet at full dimensions under the default (GSTTACO_WINO_SPLIT=1) and with the form switched off (=6, split-bf16 x6
    everywhere): both within 5e-5 of the float64 oracle; under the default exactly the layers behind a tanh -- 1, 2, 3: tanh follows
    layers 0..2 only (Taco2.py:145), so the last layer reads an unbounded BatchNorm output -- run the fp16 form."""
    from gst_tacotron_amd import synthetic, weights
    from oracle import oracle_np
    from test_gpu_parity import TOL, _model
    hp = synthetic.config_hp("cfg2")
    w = weights.synthetic_weights(hp, seed=5)
    w64 = oracle_np.cast_weights(w, np.float64)
    for B, T in ((8, 1024), (16, 1022)):
        x = np.clip(np.random.default_rng(T).normal(0, 1.5, (B, T, 80)), -4, 4).astype(np.float32)
        ref = oracle_np.postnet(hp, w64, x.astype(np.float64), np.float64)
        errs, variants = {}, {}
        for knob in ("1", "6"):
            monkeypatch.setenv("GSTTACO_WINO", "4")
            monkeypatch.setenv("GSTTACO_WINO_SPLIT", knob)
            hpv = dict(hp); hpv["Max_Step"] = 1024
            m = _model(hpv, w, B, 8, 4)
            variants[knob] = m.postnet_variants(B, T)
            errs[knob] = float(np.abs(m.postnet(x).cpu().numpy() - ref).max())
        print("\npostnet", B, T, "max-abs error vs the float64 oracle: default (fp16 x3 behind tanh) {:.3e}, x6 everywhere {:.3e}".format(
            errs["1"], errs["6"]), [capi.CONV_V_NAMES[v] for v in variants["1"]])
        assert len(variants["1"]) == 5
        assert not set(variants["6"]) & set(VH.values())
        # layers 0 (mels in) and 4 (a BatchNorm output in) run what they run without the form; 1..3 its x6 counterpart's transform
        assert variants["1"][0] == variants["6"][0] == V["WINO4_S" if T == 1022 else "WINO2_S"]
        assert variants["1"][4] == variants["6"][4]
        assert all(v in VH.values() and X6_OF[v] == v6 for v, v6 in zip(variants["1"][1:4], variants["6"][1:4]))
        assert errs["1"] <= TOL and errs["6"] <= TOL
