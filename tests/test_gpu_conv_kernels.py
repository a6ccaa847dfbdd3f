"""GPU: every kernel instantiation of the conv/GEMM dispatcher (gt_launch_conv_gemm) against the float64 reference of its contract
(oracle/conv_ref.py), through gsttaco_debug_conv_prepare / _run, at the shapes where its variant choice switches.

Each case is one production call site's call -- its weight forms (`forms`: what the site hands to the host's one argument builder,
conv_args, which gsttaco_debug_conv_run goes through as well) and its own fields -- and names the variant it must run (asserted: a
threshold change cannot move a case off its kernel silently).  Checks, where they apply:
  exact      small-integer data (|x|, |w| <= 15, exact scale / shift): every partial sum is exact in fp32 and bf16, so every
             non-Winograd variant must equal the float64 reference BITWISE (act none / relu)
  bound      Gaussian and wide-exponent data: |y - y_ref| <= C 2^-24 m + one rounding for the epilogue (m = the same sum on absolute
             values; the bf16 variants against the reference on bf16-rounded operands)
  guard      the output is pre-filled with a sentinel, with guard rows and columns [N, ldo): nothing outside [0, M) x [0, N) changes
  isolation  +Inf / NaN at frame 0 of utterance 1, or in a row past row_len: other utterances, the rest of utterance 1 and (for the
             row_len case) everything stay bitwise the same
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from gst_tacotron_amd import capi, synthetic, weights
from oracle import conv_ref
from oracle.oracle_np import bf16_round

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F = capi.CONV_FORM
V = capi.CONV_V
FP32_WINO = F["FP32"] | F["WINO2"] | F["WINO4"]                 # GSTTACO_WINO_SPLIT=0: the fp32-pipe Winograd kernels
SPLIT_WINO = FP32_WINO | F["WINO_SPLIT"]                         # finalize's default fp32 forms of a five-tap layer
GEMM_SPLIT = F["FP32"] | F["GEMM_SPLIT"]                         # a taps-1 Dense as the BiLSTM input half / Value projection take it
MIXED = F["FP32"] | F["BF16"]

# Error-bound constants in units of 2^-24 m.  C_DIRECT: the fp32 implicit GEMM, Conv2D, split GEMM and bf16 kernels (measured on the
# MI355X over this module's cases: at most 5.8 on Gaussian data, 19.9 on wide-exponent data).  C_WINO: one constant per transform,
# calibrated on the fp32-pipe kernels (largest measured: F(2,5) 7.9 Gaussian / 35.2 wide, F(4,5) 11.6 / 33.3) x 1.6, and the split x6
# kernels held to it (measured at most 24.8 / 31.8; the x3 knob 108 / 192 on Gaussian data).  A Winograd tile's outputs share their
# rounding errors, so there m is the largest magnitude over the tile's MO outputs.
C_DIRECT, C_DIRECT_WIDE = 16.0, 32.0
C_WINO = {2: 56.0, 4: 56.0}
TANH_ABS = 32 * U                                                 # gt_tanh = 1 - 2/(e^2x + 1) cancels near 0 by design (measured 12.6)
SENTINEL = -1572864.0                                            # (exact in bf16 too)
GUARD_ROWS = 5

WINO_V = {V["WINO2"]: 2, V["WINO2_S"]: 2, V["WINO2_S_X3"]: 2, V["WINO4"]: 4, V["WINO4_S"]: 4, V["WINO4_S_X3"]: 4}
X3_V = {V["WINO2_S_X3"], V["WINO4_S_X3"]}


def case(name, site, expect, B, T, cin, n, taps, forms=F["FP32"], pad=None, ldo=None, ldw=None, act=1, tokens=None, row_len=None,
         pool2=0, scale=True, shift=True, rowbias=False, res=False, xb=0, ob=0, x3=0, min_wgs=0, c2d=None, iso=False):
    return dict(name=name, site=site, expect=expect, B=B, T=T, cin=cin, n=n, taps=taps, forms=forms,
                pad=(taps - 1) // 2 if pad is None else pad, ldo=ldo or n, ldw=ldw or n, act=act, tokens=tokens, row_len=row_len,
                pool2=pool2, scale=scale, shift=shift, rowbias=rowbias, res=res, xb=xb, ob=ob, x3=x3, min_wgs=min_wgs, c2d=c2d, iso=iso)


def c2d_geo(H, W, k, stride):
    Ho, Wo = -(-H // stride), -(-W // stride)
    ph, pw = max((Ho - 1) * stride + k - H, 0) // 2, max((Wo - 1) * stride + k - W, 0) // 2
    return dict(H=H, W=W, kh=k, kw=k, stride=stride, pad_h=ph, pad_w=pw, Wo=Wo), Ho * Wo


def _cases():
    cs = []
    a = cs.append
    # ---- fp32 implicit GEMM.  N > 96 (vocoder conv bank, N = 128, ldo = the bank's concatenated width): <1,4,1,1> up to M = 16 384,
    # <2,2,1,2> above, <2,2,2,2> from 32 641
    a(case("bank_k3_M16384", "vocoder bank", V["IG_1411"], 16, 1024, 16, 128, 3, ldo=512, row_len=[1024] * 15 + [700], iso=True))
    a(case("bank_k4_M16385", "vocoder bank", V["IG_2212"], 5, 3277, 16, 128, 4, ldo=512, row_len=[3277, 0, 3277, 1000, 5], iso=True))
    a(case("bank_k8_headline", "vocoder bank", V["IG_2212"], 32, 1000, 80, 128, 8, ldo=1024))
    a(case("bank_k2_M32640", "vocoder bank", V["IG_2212"], 2, 16320, 8, 128, 2, ldo=1024))
    a(case("bank_k1_M32641", "vocoder bank", V["IG_2222"], 1, 32641, 8, 128, 1, ldo=1024, iso=False))
    a(case("bank_k5_M32641_b3", "vocoder bank", V["IG_2222"], 7, 4663, 8, 128, 5, ldo=640, row_len=[4663, 3, 4000, 0, 4663, 1, 17],
           iso=True))
    # N = 512 (postnet middle layers without Winograd): <2,2,2,2> from M = 8 065, <2,2,1,2> for 4 096 < M <= 8 064
    a(case("post_mid_M8064", "postnet (GSTTACO_WINO=0)", V["IG_2212"], 2, 4032, 64, 512, 5, act=2))
    a(case("post_mid_M8065", "postnet (GSTTACO_WINO=0)", V["IG_2222"], 5, 1613, 64, 512, 5, act=2))
    # smaller N: <4,1,1,3> for 64 < N <= 96, <4,1,1,2> for 32 < N <= 64, <4,1,1,1> below
    a(case("N97", "vocoder projection", V["IG_1411"], 3, 77, 32, 97, 3, ldw=100, ldo=100))
    a(case("N96", "vocoder projection", V["IG_4113"], 3, 77, 32, 96, 3, iso=True, row_len=[77, 40, 2]))
    a(case("N65", "postnet last (mel 65)", V["IG_4113"], 3, 77, 32, 65, 5, ldw=68, act=0, res=True))
    a(case("N64", "GST ref-enc width", V["IG_4112"], 3, 77, 32, 64, 5, iso=True, row_len=[77, 3, 50]))
    a(case("N33", "vocoder", V["IG_4112"], 3, 77, 32, 33, 3, ldw=36, ldo=40))
    a(case("N32", "encoder conv (tiny)", V["IG_4111"], 3, 77, 32, 32, 5, iso=True, row_len=[77, 77, 10]))
    # odd N with ldw (the 513-wide output Dense over ldw 516), the BiLSTM's 8H input half without planes, T < taps down to 1
    a(case("dense_513", "vocoder output Dense", V["IG_2222"], 32, 1000, 256, 513, 1, ldw=516, act=0, scale=False))
    a(case("bilstm_in_fp32", "lean BiLSTM input half (no planes)", V["IG_1411"], 3, 41, 64, 256, 1, act=0, scale=False, ldo=264))
    a(case("T1_k8", "vocoder bank, one frame", V["IG_1411"], 3, 1, 16, 128, 8, ldo=1024))
    a(case("T3_k8", "vocoder bank, T < taps", V["IG_1411"], 5, 3, 16, 128, 8, ldo=1024, iso=True, row_len=[3, 1, 0, 2, 3]))
    a(case("T2_k5_N80", "postnet, T < taps", V["IG_4113"], 3, 2, 80, 80, 5, forms=SPLIT_WINO, act=0, res=True))
    # encoder conv behind the token gather (tokens include 0 and vocab - 1), and the fused MaxPool of the first vocoder projection
    a(case("enc_tokens", "encoder conv 0 (token gather)", V["IG_1411"], 32, 128, 32, 512, 5, forms=SPLIT_WINO, tokens=149,
           row_len=[128, 1, 0] + [100] * 29, min_wgs=100))
    a(case("voc_proj_pool2", "vocoder projection 0 (pool2)", V["IG_4113"], 9, 333, 128, 80, 3, pool2=1, row_len=[333, 1, 2, 332, 0, 100, 333, 7, 64],
           iso=True))
    a(case("voc_proj_pool2_N128", "vocoder projection 0 (pool2)", V["IG_2212"], 32, 1000, 128, 128, 3, pool2=1))
    a(case("value_rowbias", "Value projection (GST rowbias)", V["IG_1411"], 7, 45, 64, 128, 1, forms=GEMM_SPLIT, act=0, scale=False,
           shift=False, rowbias=True))
    # ---- Conv2D (GST reference encoder, SAME padding, stride 2): <1,4,1,1> for N > 64, <4,1,1,2> for 32 < N <= 64, <4,1,1,1> below
    g, T2 = c2d_geo(25, 19, 3, 2)
    a(case("c2d_N32", "GST Conv2D", V["C2D_4111"], 3, T2, 16, 32, 9, c2d=g, iso=True))
    a(case("c2d_N64", "GST Conv2D", V["C2D_4112"], 3, T2, 32, 64, 9, c2d=g, iso=True))
    g1, T1 = c2d_geo(24, 10, 3, 1)
    a(case("c2d_N128_s1", "GST Conv2D", V["C2D_1411"], 2, T1, 64, 128, 9, c2d=g1, iso=True))
    # ---- split GEMM (taps 1, >= 48 workgroups): the BiLSTM input half (512 -> 8H = 2048) and the Value projection (512 -> 128)
    a(case("bilstm_in_4096", "lean BiLSTM input half", V["GEMM_SPLIT"], 32, 128, 512, 2048, 1, forms=GEMM_SPLIT, act=0, scale=False))
    a(case("bilstm_in_M129", "lean BiLSTM input half", V["GEMM_SPLIT"], 3, 43, 512, 2048, 1, forms=GEMM_SPLIT, act=0, scale=False, iso=True))
    a(case("bilstm_in_M128", "lean BiLSTM input half", V["IG_1411"], 2, 64, 512, 2048, 1, forms=GEMM_SPLIT, act=0, scale=False))
    a(case("value_M3009", "Value projection", V["GEMM_SPLIT"], 3, 1003, 512, 128, 1, forms=GEMM_SPLIT, act=0, scale=False, rowbias=True))
    a(case("value_M3008", "Value projection", V["IG_1411"], 32, 94, 512, 128, 1, forms=GEMM_SPLIT, act=0, scale=False, rowbias=True))
    # ---- Winograd (240-workgroup rule; N = 512: F(4,5) from P4 = 3 777 tiles, F(2,5) from P2 = 3 777; N = 80: 15 297)
    for tag, forms, v4, v2 in (("fp32", FP32_WINO, V["WINO4"], V["WINO2"]), ("split", SPLIT_WINO, V["WINO4_S"], V["WINO2_S"])):
        a(case("post0_F4_" + tag, "postnet conv 0 (80 -> 512)", v4, 3, 5033, 80, 512, 5, forms=forms, act=2, iso=True,
               row_len=[5033, 5000, 4]))
        a(case("post0_F2_" + tag, "postnet conv 0 (80 -> 512)", v2, 3, 5032, 80, 512, 5, forms=forms, act=2, iso=True,
               row_len=[5032, 5032, 17]))
        a(case("post4_F4_" + tag, "postnet last (512 -> 80, res)", v4, 4, 15300, 128, 80, 5, forms=forms, act=0, res=True))
        a(case("post4_F2_" + tag, "postnet last (512 -> 80, res)", v2, 4, 7650, 128, 80, 5, forms=forms, act=0, res=True))
    a(case("post0_IG_below_F2", "postnet conv 0 (80 -> 512)", V["IG_2212"], 3, 2516, 80, 512, 5, forms=SPLIT_WINO, act=2))
    a(case("post0_F2_at", "postnet conv 0 (80 -> 512)", V["WINO2_S"], 3, 2517, 80, 512, 5, forms=SPLIT_WINO, act=2))
    a(case("post4_IG_below_F2", "postnet last (512 -> 80, res)", V["IG_4113"], 4, 7646, 128, 80, 5, forms=SPLIT_WINO, act=0, res=True))
    # encoder (enc_wino 2: F(2,5) down to 100 workgroups; enc_wino 4: F(4,5) down to 60)
    a(case("enc_F2_min100", "encoder conv 1", V["WINO2_S"], 1, 3074, 512, 512, 5, forms=F["FP32"] | F["WINO2"] | F["WINO_SPLIT"],
           min_wgs=100))
    a(case("enc_IG_min100", "encoder conv 1", V["IG_1411"], 1, 3072, 512, 512, 5, forms=F["FP32"] | F["WINO2"] | F["WINO_SPLIT"],
           min_wgs=100))
    a(case("enc_F4_min60", "encoder conv 1 (enc_wino 4)", V["WINO4_S"], 4, 897, 512, 512, 5, forms=SPLIT_WINO, min_wgs=60,
           row_len=[897, 896, 600, 1], iso=True))
    a(case("enc_F2_min60", "encoder conv 1 (enc_wino 4)", V["WINO2_S"], 4, 896, 512, 512, 5, forms=SPLIT_WINO, min_wgs=60))
    # the x3 knob (GSTTACO_WINO_SPLIT=3): the negative control, must FAIL the bound
    a(case("post0_F4_x3", "postnet conv 0, x3 knob", V["WINO4_S_X3"], 3, 5033, 80, 512, 5, forms=SPLIT_WINO, act=0, x3=1))
    a(case("post4_F2_x3", "postnet last, x3 knob", V["WINO2_S_X3"], 4, 7650, 128, 80, 5, forms=SPLIT_WINO, act=0, x3=1))
    # ---- mixed precision.  bf16 five-tap: T >= 64, <4> for N > 128, <2> for 64 <= N <= 128 (postnet; the XB / OB forms are the
    # activations between bf16 layers)
    for xb in (0, 1):
        for ob in (0, 1):
            sfx = ("_XB" if xb else "") + ("_OB" if ob else "")
            a(case("c5_N129" + sfx, "postnet (mixed)", V["C5_RN4" + sfx], 3, 301, 64, 130, 5, forms=MIXED, ldw=132, act=2, xb=xb, ob=ob,
                   iso=not (xb or ob), row_len=[301, 64, 3]))
            a(case("c5_N128" + sfx, "postnet (mixed)", V["C5_RN2" + sfx], 3, 64, 80, 128, 5, forms=MIXED, act=0, xb=xb, ob=ob,
                   iso=not (xb or ob), row_len=[64, 64, 63]))
            # bf16 implicit GEMM: 256 tiles of 128 x 128 switch <1> -> <2> (N = 512: M = 8 065)
            a(case("bf16_M8065" + sfx, "vocoder projection (mixed)", V["BF16_RM2" + sfx], 5, 1613, 64, 512, 3, forms=MIXED, xb=xb, ob=ob,
                   iso=not (xb or ob)))
            a(case("bf16_M8064" + sfx, "vocoder projection (mixed)", V["BF16_RM1" + sfx], 2, 4032, 64, 512, 3, forms=MIXED, xb=xb, ob=ob,
                   iso=not (xb or ob), row_len=[4032, 1]))
    a(case("c5_T63", "postnet (mixed), T < 64", V["BF16_RM1"], 3, 63, 64, 512, 5, forms=MIXED, act=2))
    a(case("c5_N63", "five taps, N < 64", V["BF16_RM1"], 3, 100, 64, 62, 5, forms=MIXED, ldw=64, act=0, res=True))
    a(case("bf16_pool2", "vocoder projection 0 (mixed, pool2)", V["BF16_RM1"], 32, 1000, 128, 128, 3, forms=MIXED, pool2=1,
           row_len=[1000, 1, 0] + [999] * 29, iso=True))
    a(case("bf16_tokens", "encoder conv 0 (mixed, token gather)", V["BF16_RM1"], 32, 128, 32, 512, 5, forms=MIXED, tokens=149,
           row_len=[128, 1, 0] + [100] * 29))
    a(case("bf16_dense_513", "vocoder output Dense (mixed)", V["BF16_RM2"], 32, 1000, 256, 513, 1, forms=MIXED, ldw=516, act=0,
           scale=False))
    return cs


CASES = _cases()


# --------------------------------------------------------------------------------------------------------------------- the hook
class Hook:
    """One finalized context (the tiny synthetic model) used only for its gsttaco_debug_conv_* entry points."""

    def __init__(self, mixed):
        hp = synthetic.tiny_hp()
        hp["Use_Mixed_Precision"] = bool(mixed)
        self.ctx = capi.Context(hp, max_batch=2, max_tokens=8, max_ref_frames=9)
        self.ctx.load_weights(weights.synthetic_weights(hp, seed=0))
        self.ctx.finalize()
        self.lib = self.ctx.lib

    def prepare(self, w, taps, cin, n, ldw, forms, scale, shift):
        d = capi.ConvDesc(taps, cin, n, ldw, forms)
        idv = ctypes.c_int(-1)
        f32p = ctypes.POINTER(ctypes.c_float)
        w = np.ascontiguousarray(w, np.float32)
        sc = None if scale is None else np.ascontiguousarray(scale, np.float32)
        sh = None if shift is None else np.ascontiguousarray(shift, np.float32)
        self.ctx.check(self.lib.gsttaco_debug_conv_prepare(
            self.ctx.handle, ctypes.byref(d), w.ctypes.data_as(f32p), None if sc is None else sc.ctypes.data_as(f32p),
            None if sh is None else sh.ctypes.data_as(f32p), ctypes.byref(idv)))
        return idv.value

    def run(self, wid, call, x, out, tokens=None, row_len=None, rowbias=None, res=None, stream=None):
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())     # noqa: E731
        v = ctypes.c_int(-2)
        s = ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        self.ctx.check(self.lib.gsttaco_debug_conv_run(self.ctx.handle, wid, ctypes.byref(call), p(x), p(tokens), p(row_len), p(rowbias),
                                                       p(res), p(out), ctypes.byref(v), s))
        return v.value


_hooks = {}


def hook(mixed):
    if mixed not in _hooks:
        _hooks[mixed] = Hook(mixed)
    return _hooks[mixed]


def teardown_module(module):
    torch.cuda.synchronize()
    for h in _hooks.values():
        h.ctx.close()
    _hooks.clear()


# --------------------------------------------------------------------------------------------------------------------- data
def make_data(c, kind, rng):
    """Host data of one case: dict(x, w, scale, shift, rowbias, res, tokens, row_len) as float64 / int32 arrays."""
    B, T, cin, n, taps = c["B"], c["T"], c["cin"], c["n"], c["taps"]
    rows = c["tokens"] if c["tokens"] else (B * T if c["c2d"] is None else B * c["c2d"]["H"] * c["c2d"]["W"])
    K = taps * cin

    def draw(shape):
        if kind == "exact":
            return rng.integers(-15, 16, shape).astype(np.float64)
        v = rng.standard_normal(shape)
        if kind == "wide":
            v = v * 2.0 ** rng.integers(-8, 1, shape)
        return v

    d = dict(x=draw((rows, cin)), w=np.zeros((K, c["ldw"])))
    d["w"][:, :n] = draw((K, n))
    if c["ldw"] > n:
        d["w"][:, n:] = np.nan          # columns past N must never be read
    if kind == "exact":
        d["scale"] = 2.0 ** rng.integers(-2, 2, n) * rng.choice([-1, 1], n) if c["scale"] else None
        d["shift"] = rng.integers(-64, 65, n).astype(np.float64) if c["shift"] else None
        d["rowbias"] = rng.integers(-64, 65, (B, n)).astype(np.float64) if c["rowbias"] else None
        d["res"] = rng.integers(-64, 65, (B * T, n)).astype(np.float64) if c["res"] else None
    else:
        d["scale"] = rng.uniform(0.5, 1.5, n) * rng.choice([-1, 1], n) if c["scale"] else None
        d["shift"] = rng.standard_normal(n) if c["shift"] else None
        d["rowbias"] = rng.standard_normal((B, n)) if c["rowbias"] else None
        d["res"] = rng.standard_normal((B * T, n)) if c["res"] else None
    if c["scale"] and kind != "exact":
        d["w"][:, :n] /= np.sqrt(K)
    d["tokens"] = None
    if c["tokens"]:
        tk = rng.integers(0, c["tokens"], (B, T)).astype(np.int32)
        tk.flat[0], tk.flat[-1] = 0, c["tokens"] - 1
        d["tokens"] = tk
    d["row_len"] = None if c["row_len"] is None else np.asarray(c["row_len"], np.int32)
    return d


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def run_case(c, d, act=None, x_override=None, row_len=None):
    """Runs one case on the device; returns (variant, out [M, N] float64, the whole output buffer as raw bits)."""
    mixed = bool(c["forms"] & F["BF16"])
    h = hook(mixed)
    key = "_wid"
    if key not in d:
        d[key] = h.prepare(d["w"], c["taps"], c["cin"], c["n"], c["ldw"], c["forms"],
                           d["scale"] if d["scale"] is not None else None, d["shift"])
    dev = torch.device("cuda")
    x = torch.from_numpy(np.asarray(x_override if x_override is not None else d["x"], np.float32)).to(dev)
    if c["xb"]:
        x = x.to(torch.bfloat16)
    M, N, ldo = c["B"] * c["T"], c["n"], c["ldo"]
    odt = torch.bfloat16 if c["ob"] else torch.float32
    out = torch.full((M + GUARD_ROWS, ldo), SENTINEL, dtype=odt, device=dev)
    t = lambda a, dt=torch.float32: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)   # noqa: E731
    rl = d["row_len"] if row_len is None else row_len
    call = capi.ConvCall()
    call.forms, call.B, call.T, call.pad_before = c["forms"], c["B"], c["T"], c["pad"]
    call.act = c["act"] if act is None else act
    call.ldo, call.pool2, call.x_bf16, call.out_bf16 = ldo, c["pool2"], c["xb"], c["ob"]
    call.wino_x3, call.wino_min_wgs = c["x3"], c["min_wgs"]
    if c["c2d"] is not None:
        g = c["c2d"]
        call.conv2d, call.H, call.W, call.Wo, call.kw = 1, g["H"], g["W"], g["Wo"], g["kw"]
        call.stride, call.pad_h, call.pad_w, call.xb = g["stride"], g["pad_h"], g["pad_w"], g["H"] * g["W"] * c["cin"]
    v = h.run(d[key], call, x, out, tokens=t(d["tokens"], torch.int32), row_len=t(rl, torch.int32), rowbias=t(d["rowbias"]),
              res=t(d["res"]))
    torch.cuda.synchronize()
    o = out.float().cpu().numpy().astype(np.float64)
    raw = out.view(torch.int16).cpu().numpy() if c["ob"] else out.view(torch.int32).cpu().numpy()
    # guard band: rows past M, columns [N, ldo)
    assert np.all(o[M:] == SENTINEL), "{}: a guard row was written".format(c["name"])
    if ldo > N:
        assert np.all(o[:M, N:] == SENTINEL), "{}: a column in [N, ldo) was written".format(c["name"])
    return v, o[:M, :N], raw


def reference(c, d, act=None, row_len=None):
    bf = bool(c["forms"] & F["BF16"])
    x = d["x"]
    if c["xb"] or bf:
        x = bf16_round(x.astype(np.float32)).astype(np.float64)
    kw = dict(pad_before=c["pad"], tokens=d["tokens"], row_len=d["row_len"] if row_len is None else row_len, pool2=bool(c["pool2"]),
              scale=None if d["scale"] is None else f32(d["scale"]), shift=None if d["shift"] is None else f32(d["shift"]),
              rowbias=None if d["rowbias"] is None else f32(d["rowbias"]), act=c["act"] if act is None else act,
              res=None if d["res"] is None else f32(d["res"]), ldw=c["ldw"], bf16=bf)
    if c["c2d"] is not None:
        kw = dict(scale=kw["scale"], shift=kw["shift"], act=kw["act"], conv2d=c["c2d"])
    y, m = conv_ref.conv_gemm_ref(f32(x), f32(d["w"][:, :c["n"]]), c["B"], c["T"], c["cin"], c["n"], c["taps"],
                                  **{k: v for k, v in kw.items() if k != "ldw"})
    return y, m


def tile_magnitude(c, m, mo):
    """m -> the largest m over each Winograd tile (MO consecutive outputs of one utterance)."""
    B, T, N = c["B"], c["T"], m.shape[-1]
    Tp = -(-T // mo) * mo
    mp = np.zeros((B, Tp, N))
    mp[:, :T] = m.reshape(B, T, N)
    mt = mp.reshape(B, Tp // mo, mo, N).max(axis=2, keepdims=True)
    return np.broadcast_to(mt, (B, Tp // mo, mo, N)).reshape(B, Tp, N)[:, :T].reshape(B * T, N)


def bound(c, kind, y, m, variant, act):
    if variant in WINO_V:
        C = C_WINO[WINO_V[variant]]
        m = tile_magnitude(c, m, WINO_V[variant])
    else:
        C = C_DIRECT_WIDE if kind == "wide" else C_DIRECT
    tol = C * U * m + 2 * U * np.abs(y)
    if act == 2:
        tol = tol + TANH_ABS
    if c["ob"]:
        tol = tol + 2.0 ** -8 * np.abs(y)
    return C, tol


# --------------------------------------------------------------------------------------------------------------------- tests
def test_case_table_reaches_every_variant():
    assert {c["expect"] for c in CASES} == set(V.values())
    assert len({c["name"] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_conv_kernel_case(c):
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    report = []
    # exact data: bitwise (every non-Winograd variant, act none and relu)
    if c["expect"] not in WINO_V:
        d = make_data(c, "exact", rng)
        for act in (0, 1):
            v, y, _ = run_case(c, d, act=act)
            assert v == c["expect"], "{} ({}): ran {}, expected {}".format(c["name"], c["site"], capi.CONV_V_NAMES.get(v, v),
                                                                       capi.CONV_V_NAMES[c["expect"]])
            yr, _ = reference(c, d, act=act)
            yr = f32(bf16_round(yr.astype(np.float32))) if c["ob"] else f32(yr)
            bad = np.argwhere(y != yr)
            assert bad.size == 0, "{}: {} words differ on exact data (act {}), first {} {} vs {}".format(
                c["name"], len(bad), act, bad[0], y[tuple(bad[0])], yr[tuple(bad[0])])
        report.append("exact bitwise")
    # error bound on Gaussian and wide-exponent data
    for kind in ("gauss", "wide"):
        d = make_data(c, kind, rng)
        v, y, _ = run_case(c, d)
        assert v == c["expect"], (c["name"], capi.CONV_V_NAMES.get(v, v))
        yr, m = reference(c, d)
        C, tol = bound(c, kind, yr, m, v, c["act"])
        if v in WINO_V:
            m = tile_magnitude(c, m, WINO_V[v])
        assert np.all(np.isfinite(y)), c["name"]
        ratio = float(np.max((np.abs(y - yr) - (tol - C * U * m)) / (U * np.maximum(m, 1e-30))))
        report.append("{} {:.2f} units (C {})".format(kind, ratio, C))
        if v in X3_V:
            continue
        worst = np.unravel_index(np.argmax(np.abs(y - yr) - tol), y.shape)
        assert np.all(np.abs(y - yr) <= tol), "{} ({}): {} data, {:.2f} units of 2^-24 m > C = {} at {}: {} vs {}".format(
            c["name"], capi.CONV_V_NAMES[v], kind, ratio, C, worst, y[worst], yr[worst])
    if c["expect"] in X3_V:
        # the negative control: the reduced form must exceed the bound the x6 form holds on the same case
        d = make_data(c, "gauss", rng)
        v, y, _ = run_case(c, d)
        yr, m = reference(c, d)
        _, tol = bound(c, "gauss", yr, m, v, c["act"])
        assert np.any(np.abs(y - yr) > tol), "{}: the x3 form passed the x6 bound: the bound cannot tell them apart".format(c["name"])
        report.append("x3 exceeds its bound (control)")
    print("\n{:24s} {:34s} {:14s} {}".format(c["name"], c["site"], capi.CONV_V_NAMES[c["expect"]], "; ".join(report)))


ISO_CASES = [c for c in CASES if c["iso"]]


@pytest.mark.parametrize("c", ISO_CASES, ids=[c["name"] for c in ISO_CASES])
@pytest.mark.parametrize("poison", [np.inf, np.nan], ids=["inf", "nan"])
def test_conv_kernel_nonfinite_isolation(c, poison):
    """+Inf / NaN at frame 0 of utterance 1 changes nothing outside utterance 1's footprint; one past row_len changes nothing."""
    assert c["B"] >= 2 and not c["tokens"]
    rng = np.random.default_rng(7)
    d = make_data(c, "gauss", rng)
    v, y0, raw0 = run_case(c, d)
    assert v == c["expect"]
    B, T, cin = c["B"], c["T"], c["cin"]
    per = T if c["c2d"] is None else c["c2d"]["H"] * c["c2d"]["W"]
    x = d["x"].copy()
    x[per] = poison                               # frame / pixel 0 of utterance 1
    _, _, raw1 = run_case(c, d, x_override=x)
    a0, a1 = raw0[:B * T].reshape(B, T, -1), raw1[:B * T].reshape(B, T, -1)
    for b in range(B):
        if b != 1:
            diff = np.argwhere(a0[b] != a1[b])
            assert diff.size == 0, "{} ({}): {} at utterance 1 frame 0 changed utterance {} (first at frame {})".format(
                c["name"], capi.CONV_V_NAMES[v], poison, b, diff[0][0])
    if c["c2d"] is None:
        far = c["taps"] + 4 + (1 if c["pool2"] else 0)
        diff = np.argwhere(a0[1, far:] != a1[1, far:])
        assert diff.size == 0, "{}: {} at frame 0 changed frame {} of its own utterance".format(c["name"], poison, far + diff[0][0])
    # one row at or beyond row_len: nothing at all may change
    rl = d["row_len"]
    if rl is not None and c["c2d"] is None:
        b = int(np.argmax(rl < T)) if np.any(rl < T) else None
        if b is not None:
            x = d["x"].copy()
            x[b * T + max(int(rl[b]), 0)] = poison
            if int(rl[b]) + 1 < T:
                x[b * T + T - 1] = poison
            _, _, raw2 = run_case(c, d, x_override=x)
            diff = np.argwhere(raw0 != raw2)
            assert diff.size == 0, "{}: {} past row_len of utterance {} changed the output at {}".format(c["name"], poison, b, diff[0])


def _coherent_operand(rng, shape):
    """h + m + l from bf16 parts, all positive: h in [1, 2) (ulp 2^-7), m in [0.75, 1) 2^-8 (just under half an ulp of h; ulp 2^-16),
    l in [0.75, 1) 2^-17 on the fp32 grid (just under half an ulp of m): the sum is an fp32 number that splits back into h, m, l."""
    h = 1.0 + rng.integers(0, 128, shape) * 2.0 ** -7
    hm = 2.0 ** -8 * (0.75 + rng.integers(0, 64, shape) * 2.0 ** -8)
    lo = 2.0 ** -23 * rng.integers(48, 64, shape)
    return h + hm + lo


def test_split_gemm_coherent_residuals():
    """Every dropped plane product adds with one sign on this data: x6 leaves ~1 unit of 2^-24 m, a missing mm / hl / lh 128-256.
    K = 64, the kernel's shortest: the fp32 accumulation's own rounding is one-sided on all-positive data too and grows with K (64.6
    units at K = 512), where a lost plane product costs the same 128-256 units at any K."""
    c = dict([k for k in CASES if k["name"] == "bilstm_in_M129"][0], cin=64)
    rng = np.random.default_rng(11)
    d = make_data(c, "gauss", rng)
    K, n = c["cin"], c["n"]
    d["x"] = _coherent_operand(rng, d["x"].shape)
    w = _coherent_operand(rng, (K, n))
    d["w"] = w
    d["shift"] = np.zeros(n)
    assert np.all(f32(d["x"]) == d["x"]) and np.all(f32(w) == w)
    v, y, _ = run_case(c, d)
    assert v == V["GEMM_SPLIT"]
    yr, m = reference(c, d)
    units = float(np.max(np.abs(y - yr) / (U * m)))
    print("\nsplit GEMM on coherent residuals: {:.2f} units of 2^-24 m (bound {})".format(units, C_DIRECT))
    assert units <= C_DIRECT


def test_split_gemm_concurrent_streams_bitwise():
    """gt_gemm_split_kernel at the BiLSTM-input shape, 200 calls over 4 streams in rounds: every output equals the lone result."""
    c = [k for k in CASES if k["name"] == "bilstm_in_4096"][0]
    rng = np.random.default_rng(5)
    d = make_data(c, "gauss", rng)
    h = hook(False)
    wid = h.prepare(d["w"], 1, c["cin"], c["n"], c["ldw"], c["forms"], None, d["shift"])
    dev = torch.device("cuda")
    x = torch.from_numpy(d["x"].astype(np.float32)).to(dev)
    call = capi.ConvCall()
    call.forms, call.B, call.T, call.ldo = c["forms"], c["B"], c["T"], c["n"]
    M = c["B"] * c["T"]
    lone = torch.empty((M, c["n"]), device=dev)
    assert h.run(wid, call, x, lone) == V["GEMM_SPLIT"]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(4)]
    per_round, total = 20, 200
    outs = [torch.empty_like(lone) for _ in range(per_round)]
    bad = 0
    for r in range(total // per_round):
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            o.fill_(SENTINEL)
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            h.run(wid, call, x, o, stream=streams[i % 4])
        torch.cuda.synchronize()
        bad += sum(int(not torch.equal(o.view(torch.int32), lone.view(torch.int32))) for o in outs)
    assert bad == 0, "{} of {} concurrent calls differed from the lone result".format(bad, total)


@pytest.mark.parametrize("mixed", [False, True], ids=["fp32", "mixed"])
def test_conv_past_2gib_input(mixed):
    """x of M * Cin * 4 >= 2^31 bytes: Winograd, split and five-tap decline (their buffer resources cannot span it); the implicit GEMM
    (fp32) and the bf16 GEMM's non-buffer gather (mixed) are right on rows on both sides of the 2 GiB offset."""
    B, T, cin, n, taps = 1, 2 ** 20 + 17, 512, 80, 5
    assert B * T * cin * 4 >= 2 ** 31
    forms = MIXED if mixed else SPLIT_WINO
    c = case("big", "postnet last, 2 GiB input", V["BF16_RM2"] if mixed else V["IG_4113"], B, T, cin, n, taps, forms=forms, act=0)
    rng = np.random.default_rng(3)
    w = rng.standard_normal((taps * cin, n)) / np.sqrt(taps * cin)
    sc, sh = rng.uniform(0.5, 1.5, n), rng.standard_normal(n)
    h = hook(mixed)
    wid = h.prepare(w, taps, cin, n, n, forms, sc, sh)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.randn((B * T, cin), device=dev, generator=g)
    out = torch.full((B * T + GUARD_ROWS, n), SENTINEL, device=dev)
    call = capi.ConvCall()
    call.forms, call.B, call.T, call.pad_before, call.act, call.ldo = forms, B, T, 2, 0, n
    v = h.run(wid, call, x, out)
    torch.cuda.synchronize()
    assert v == c["expect"], capi.CONV_V_NAMES.get(v, v)
    edge = 2 ** 31 // (4 * cin)
    spans = [(0, 8), (edge - 8, edge + 8), (T - 8, T)]
    for lo, hi in spans:
        a, b2 = max(lo - 2, 0), min(hi + 2, T)
        xs = x[a:b2].cpu().numpy().astype(np.float64)
        # the window's rows as a batch of one utterance; rows outside [0, T) read as zero, so a window at the edge pads the same way
        sub = dict(x=xs, w=w, scale=sc, shift=sh, rowbias=None, res=None, tokens=None, row_len=None)
        cc = dict(c, B=1, T=b2 - a, ldw=n, pad=2)
        yr, m = reference(cc, sub)
        yr, m = yr[lo - a:hi - a], m[lo - a:hi - a]
        y = out[lo:hi].cpu().numpy().astype(np.float64)
        C, tol = bound(c, "gauss", yr, m, v, 0)
        ratio = float(np.max(np.abs(y - yr) / (U * m)))
        print("\n2 GiB input ({}): rows {}..{}: {} {:.2f} units".format("mixed" if mixed else "fp32", lo, hi, capi.CONV_V_NAMES[v], ratio))
        assert np.all(np.abs(y - yr) <= tol), (lo, hi, ratio)
    assert torch.all(out[B * T:] == SENTINEL)
    del x, out
    torch.cuda.empty_cache()
