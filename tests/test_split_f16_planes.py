"""CPU: the bounded-input Winograd form (conv_wino_split.hip, plane mode fp16 x3) without a GPU.

1. The host plane builder (gsttaco.cpp wino_split_h_planes, through gsttaco_debug_wino_h_planes -- the function finalize runs): per
   column power-of-two scaling SU[n], two fp16 planes, on a random column, an all-zero column, a 2^-20 column and a 2^6 column.
2. A numpy emulation of the kernel's arithmetic on one transform-domain GEMM (K = 512): the F(4,5) input transform's row of sum 15 in
   fp32 with the factor 2^SV folded in, hi = fp16(v), lo = fp16(v - hi), the library's planes of U, the products hh, hl, lh of every
   16 k summed exactly and rounded into ONE fp32 accumulator, times 2^-(SV + SU[n]) -- against float64, beside an emulation of the
   fp32 MFMA chain (four products per rounding) on the same data.  Each case with fp16 subnormals kept and flushed to zero.
   Measured here (units of 2^-24 sum|v u|, max over 512 x 32 outputs; subnormals kept / flushed):
     tanh of N(0, 1.5)   fp32 chain 1.66, fp16 x3 1.72 / 1.72
     all +-1 (V = 15)    fp32 chain 1.49, fp16 x3 1.06 / 1.06
     |x| <= 2^-12        fp32 chain 1.66, fp16 x3 2.22 / 39.9; absolute, in units of 2^-24 sum|u|: 0.0019 / 0.032 (bound 1)
"""
import ctypes

import numpy as np
import pytest

from gst_tacotron_amd import capi

BT4_ROW15 = np.array([0.0, 2.0, 4.0, -2.5, -5.0, 0.5, 1.0, 0.0])        # wino_common.h Wino<4>::bt row 3: absolute sum 15
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    from gst_tacotron_amd import build
    build.build()
    return capi.load_library()


def build_planes(lib, u, wino_cin=None, npad=None):
    """u [al][cin][cout] float64 -> (hi, lo [al][cout][cin] float64 values of the fp16 planes, raw planes, su [cout], sv)."""
    al, cin, cout = u.shape
    wino_cin, npad = wino_cin or cin, npad or cout
    u = np.ascontiguousarray(u, np.float64)
    planes = np.full((al, 2, npad, wino_cin), 0x7e00, np.uint16)          # (pre-filled with NaN bits: the builder writes all of it)
    su = np.full(cout, -12345, np.int32)
    sv = ctypes.c_int32(-1)
    rc = lib.gsttaco_debug_wino_h_planes(u.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), al, cin, wino_cin, cout, npad,
                                         planes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                         su.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(sv))
    assert rc == 0
    val = planes.view(np.float16).astype(np.float64)
    return val[:, 0, :cout, :cin], val[:, 1, :cout, :cin], planes, su, sv.value


def test_plane_builder_columns(lib):
    rng = np.random.default_rng(0)
    al, cin, cout = 8, 40, 7
    u = rng.standard_normal((al, cin, cout)) * 0.05
    u[:, :, 1] = 0.0                                                    # an all-zero column
    u[:, :, 2] = rng.uniform(-1, 1, (al, cin)) * 2.0 ** -20             # magnitude 2^-20
    u[:, :, 3] = rng.uniform(-1, 1, (al, cin)) * 2.0 ** 6               # magnitude 2^6
    u[0, 0, 4] = 0.25                                                   # a column whose largest entry is a power of two
    u[:, :, 4] = np.clip(u[:, :, 4], -0.25, 0.25)
    u[3, 5, 5] *= 2.0 ** -30                                            # one entry far below its column
    hi, lo, planes, su, sv = build_planes(lib, u, wino_cin=64, npad=128)
    assert sv == 11                                                     # 15 . 1 . 2^11 = 30 720 <= 2^15 < 15 . 2^12
    assert su.dtype == np.int32 and su[1] == 0
    raw = planes.view(np.float16)
    assert np.all(np.isfinite(raw))
    mx = np.abs(u).max(axis=(0, 1))
    for n in range(cout):
        if mx[n] > 0:
            assert su[n] == int(np.floor(np.log2(2.0 ** 14 / mx[n]))), n
            assert 2.0 ** 13 < mx[n] * 2.0 ** su[n] <= 2.0 ** 14
    assert np.abs(hi).max() < 2.0 ** 15
    rec = (hi + lo) * 2.0 ** -su.astype(np.float64)[None, :, None]            # [al][cout][cin]
    ut = u.transpose(0, 2, 1)
    tol = np.maximum(2.0 ** -22 * np.abs(ut), 2.0 ** -25 * mx[None, :, None])
    assert np.all(np.abs(rec - ut) <= tol), float(np.max(np.abs(rec - ut) / np.maximum(tol, 1e-300)))
    # the zero column, the padding columns and the padding channels are zero planes
    assert not planes[:, :, 1].any() and not planes[:, :, cout:].any() and not planes[:, :, :, cin:].any()
    # hi is the round-to-nearest fp16 of the scaled value, lo of what is left
    s = ut * 2.0 ** su.astype(np.float64)[None, :, None]
    with np.errstate(over="raise"):
        assert np.array_equal(hi, s.astype(np.float16).astype(np.float64))
        assert np.array_equal(lo, (s - hi).astype(np.float16).astype(np.float64))


def test_plane_builder_rejects_bad_geometry(lib):
    u = np.zeros((1, 4, 4))
    p = np.zeros(1 * 2 * 4 * 4, np.uint16)
    su = np.zeros(4, np.int32)
    args = (u.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1, 4)
    tail = (p.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), su.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None)
    assert lib.gsttaco_debug_wino_h_planes(*args, 3, 4, 4, *tail) != 0          # wino_cin < cin
    assert lib.gsttaco_debug_wino_h_planes(*args, 4, 4, 3, *tail) != 0          # npad < cout
    assert lib.gsttaco_debug_wino_h_planes(*args, 4, 4, 4, *tail) == 0


# --------------------------------------------------------------------------------------------------------------------- emulation
def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def flush16(a):
    """fp16 values (as float64) with the subnormals flushed to zero"""
    return np.where(np.abs(a) < 2.0 ** -14, 0.0, a)


def transform_fp32(x, scale):
    """v = sum_tap (bt[tap] scale) x[tap] as the kernel's chain of fp32 fmas (an fma: the exact product, one rounding per tap)"""
    v = np.zeros(x.shape[:-1])
    for tap in range(8):
        if BT4_ROW15[tap] != 0.0:
            v = f32(BT4_ROW15[tap] * scale * x[..., tap] + v)            # (float64 holds the product and the sum exactly enough: 24 + 24 bits)
    return v


def chain(pairs, per):
    """sum over k in blocks of `per`: each listed product (a [rows][K], b [K][N]) summed over the block in float64, then rounded into ONE
    fp32 accumulator, in the order listed"""
    rows, K = pairs[0][0].shape
    acc = np.zeros((rows, pairs[0][1].shape[1]))
    for k0 in range(0, K, per):
        for a, b in pairs:
            acc = f32(acc + a[:, k0:k0 + per] @ b[k0:k0 + per])
    return acc


def emulate(lib, x, u, flush):
    """x [rows][K][8 taps], u [K][N] float64 -> (new form, fp32 chain, float64 reference, sum|v u|, max|v 2^SV|, sum|u|)"""
    hi_u, lo_u, _, su, sv = build_planes(lib, u[None])
    hi_u, lo_u = hi_u[0].T, lo_u[0].T                                   # [K][N]
    vs = transform_fp32(x, 2.0 ** sv)                                   # the scaled transform, fp32
    hi_v = vs.astype(np.float16).astype(np.float64)
    lo_v = (vs - hi_v).astype(np.float16).astype(np.float64)
    if flush:
        hi_v, lo_v, hi_u, lo_u = flush16(hi_v), flush16(lo_v), flush16(hi_u), flush16(lo_u)
    acc = chain([(hi_v, hi_u), (hi_v, lo_u), (lo_v, hi_u)], 16)         # hh, hl, lh per 16 k into one accumulator
    y_new = acc * 2.0 ** -(sv + su.astype(np.float64))[None, :]
    v = transform_fp32(x, 1.0)                                          # (= vs 2^-SV exactly)
    assert np.array_equal(v * 2.0 ** sv, vs)
    y_chain = chain([(v, f32(u))], 4)                                   # the fp32 MFMA: four products per rounding
    ref = v @ u
    return y_new, y_chain, ref, np.abs(v) @ np.abs(u), float(np.abs(vs).max()), np.abs(u).sum(axis=0)


def make_inputs(kind, rng, rows, K):
    if kind == "tanh":
        return f32(np.tanh(rng.normal(0, 1.5, (rows, K, 8))))
    if kind == "saturated":
        s = np.where(BT4_ROW15 < 0, -1.0, 1.0)
        return np.broadcast_to(s, (rows, K, 8)) * rng.choice([-1.0, 1.0], (rows, K, 1))
    return f32(rng.uniform(-1, 1, (rows, K, 8)) * 2.0 ** -12)


@pytest.mark.parametrize("flush", [False, True], ids=["subnormals", "flushed"])
@pytest.mark.parametrize("kind", ["tanh", "saturated", "tiny"])
def test_kernel_arithmetic_emulation(lib, kind, flush):
    rng = np.random.default_rng(3)
    rows, K, N = 512, 512, 32
    x = make_inputs(kind, rng, rows, K)
    u = rng.normal(0, 0.05, (K, N)) * np.exp(rng.uniform(np.log(0.01), np.log(4.0), N))[None, :]
    y_new, y_chain, ref, m, vmax, usum = emulate(lib, x, u, flush)
    assert vmax <= 30720.0
    if kind == "saturated":
        assert vmax == 30720.0                                           # the edge itself
    e_new, e_chain = float(np.max(np.abs(y_new - ref) / (U24 * m))), float(np.max(np.abs(y_chain - ref) / (U24 * m)))
    a_new = float(np.max(np.abs(y_new - ref) / (U24 * usum[None, :])))
    print("\n{} flush {}: fp32 chain {:.2f}, fp16 x3 {:.2f} units of 2^-24 sum|v u|; abs {:.3g} of 2^-24 sum|u|".format(
        kind, flush, e_chain, e_new, a_new))
    # (1.6: the factor C_WINO was calibrated with.)  Tiny inputs with the subnormals FLUSHED are held to the absolute bound alone: below
    # |v 2^SV| = 2^-3 a low plane is a subnormal, so a flushing matrix unit keeps 11 bits of such a value -- an error of at most
    # 2^-14 2^-SV = 2^-25 per unit of |u|, against a full-scale input of 1: nothing, but many units of sum|v u| when EVERY input is tiny
    if not (kind == "tiny" and flush):
        assert e_new <= 1.6 * e_chain
    if kind == "tiny":
        assert np.all(np.abs(y_new - ref) < U24 * usum[None, :])
