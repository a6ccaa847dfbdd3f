"""ctypes binding of include/gsttaco.h (the C-ABI of the HIP hot path).

This is the stub a maintainer of the reference would add in place of the Keras
functional model (reference Model.py:145-156); see INTEGRATION.md.  There is no CPU
fallback: a missing library raises ImportError here and a missing GPU surfaces as
GSTTACO_E_NO_DEVICE from gsttaco_finalize_weights.
"""
import ctypes
import os

import numpy as np
import torch  # noqa: F401  -- must be imported BEFORE the dlopen below: torch bundles the HIP runtime that owns the
#                     tensors/streams handed to the C-ABI, and libgsttaco.so has to bind to that same libamdhip64

from .hparams import Dims

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgsttaco.so")

MAX_LAYERS = 8
ABI_VERSION = 14
ATT_CODES = {"BMA": 0, "SMA": 1, "LSA": 2}

# every symbol include/gsttaco.h declares
EXPORTED_SYMBOLS = (
    "gsttaco_abi_version", "gsttaco_create", "gsttaco_destroy", "gsttaco_last_error",
    "gsttaco_num_weights", "gsttaco_weight_info", "gsttaco_load_weight", "gsttaco_finalize_weights",
    "gsttaco_encode", "gsttaco_gst", "gsttaco_decode", "gsttaco_postnet", "gsttaco_vocoder", "gsttaco_inference_step",
    "gsttaco_mel_frontend", "gsttaco_mel_basis", "gsttaco_griffin_lim", "gsttaco_crc32c",
    "gsttaco_set_profiling", "gsttaco_get_profile", "gsttaco_lstm_launch_bytes", "gsttaco_debug_stamps", "gsttaco_decode_plan", "gsttaco_debug_randomness",
    "gsttaco_set_graph_policy", "gsttaco_graph_cache_size", "gsttaco_debug_handoff_error", "gsttaco_debug_raise_handoff_error", "gsttaco_debug_counters",
    "gsttaco_synchronize", "gsttaco_debug_conv_prepare", "gsttaco_debug_conv_run",
    "gsttaco_gst_ex", "gsttaco_style_compose", "gsttaco_inference_step_styled",
    "gsttaco_decode_forced", "gsttaco_inference_step_forced", "gsttaco_forced_durations",
    "gsttaco_fill_randomness", "gsttaco_utterance_report",
    "gsttaco_losses", "gsttaco_feature_frontend",
    "gsttaco_postnet_variants", "gsttaco_debug_wino_h_planes",
    "gsttaco_encoder_variants", "gsttaco_vocoder_variants",
    "gsttaco_decode_plan_fields",
    "gsttaco_mel_dtw",
    "gsttaco_resample",
    "gsttaco_pitch", "gsttaco_pitch_errors",
    "gsttaco_style_affinities", "gsttaco_style_map",
    "gsttaco_melgan_configure", "gsttaco_melgan_num_weights", "gsttaco_melgan_weight_info", "gsttaco_melgan_load_weight",
    "gsttaco_melgan_finalize", "gsttaco_melgan", "gsttaco_melgan_plan", "gsttaco_melgan_debug_stage",
    "gsttaco_waveglow_configure", "gsttaco_waveglow_num_weights", "gsttaco_waveglow_weight_info", "gsttaco_waveglow_load_weight",
    "gsttaco_waveglow_finalize", "gsttaco_waveglow_noise", "gsttaco_waveglow", "gsttaco_waveglow_plan", "gsttaco_waveglow_debug_stage",
    "gsttaco_hifigan_configure", "gsttaco_hifigan_num_weights", "gsttaco_hifigan_weight_info", "gsttaco_hifigan_load_weight",
    "gsttaco_hifigan_finalize", "gsttaco_hifigan", "gsttaco_hifigan_plan", "gsttaco_hifigan_debug_stage",
    "gsttaco_hifigan_set_operands", "gsttaco_hifigan_debug_buffer",
)
# gsttaco_hifigan_plan: ints per launch (kind, channels, taps, dilation, tile, form, rate, lds), the launch kinds, and the size of its array
HIFIGAN_PLAN_FIELDS = ("kind", "channels", "taps", "dilation", "tile", "form", "rate", "lds")
HIFIGAN_KINDS = ("in", "up", "conv", "out")
HIFIGAN_PLAN_INTS = 3 + 8 * 522
HIFIGAN_MAX_DILATIONS = 4
# gsttaco_hifigan_set_operands: the MFMA's operand form, by the name Load_HiFiGAN takes, and gsttaco_hifigan_debug_buffer's buffers
HIFIGAN_OPERANDS = {"float32": 0, "bfloat16": 1, "float16": 2}
HIFIGAN_BUFFERS = ("sum", "up", "a", "b")
# gsttaco_waveglow_plan: ints per launch (kind, channels, tile, form, unit, lds), the launch kinds, and the size of its array
WAVEGLOW_PLAN_FIELDS = ("kind", "channels", "tile", "form", "unit", "lds")
WAVEGLOW_KINDS = ("up", "layer", "flow")
WAVEGLOW_PLAN_INTS = 3 + 6 * 354
# gsttaco_melgan_plan: ints per launch (kind, channels, tile, form, rate, lds), the launch kinds, and the size of its array
MELGAN_PLAN_FIELDS = ("kind", "channels", "tile", "form", "rate", "lds")
MELGAN_KINDS = ("in", "up", "res", "out")
MELGAN_PLAN_INTS = 3 + 6 * 74
# GSTTACO_PLAN_*: the fields gsttaco_decode_plan_fields fills, in order
PLAN_FIELDS = ("persist", "persist_bf16", "fused", "lean_front", "lean_rec", "z0", "fuse12", "lean_x0", "lean_x1", "co_tiles", "lean_proj",
               "mirror", "dec_padded", "pj_tiles")

# GSTTACO_CONV_V_*: the conv/GEMM dispatcher's kernel instantiations (gsttaco_debug_conv_run reports which one ran)
CONV_V = {
    "IG_1411": 0, "IG_2212": 1, "IG_2222": 2, "IG_4113": 3, "IG_4112": 4, "IG_4111": 5,
    "C2D_1411": 6, "C2D_4112": 7, "C2D_4111": 8,
    "WINO4": 9, "WINO2": 10, "WINO4_S": 11, "WINO2_S": 12, "WINO4_S_X3": 13, "WINO2_S_X3": 14,
    "GEMM_SPLIT": 15,
    "C5_RN4": 16, "C5_RN4_XB": 17, "C5_RN4_OB": 18, "C5_RN4_XB_OB": 19,
    "C5_RN2": 20, "C5_RN2_XB": 21, "C5_RN2_OB": 22, "C5_RN2_XB_OB": 23,
    "BF16_RM2": 24, "BF16_RM2_XB": 25, "BF16_RM2_OB": 26, "BF16_RM2_XB_OB": 27,
    "BF16_RM1": 28, "BF16_RM1_XB": 29, "BF16_RM1_OB": 30, "BF16_RM1_XB_OB": 31,
}
CONV_V_INVALID = -1
# GSTTACO_VOC_*: the kinds of GEMM gsttaco_vocoder_variants reports, in the order the vocoder enqueues them
VOC_KINDS = {"bank": 0, "proj": 1, "proj_dense": 2, "highway_in": 3, "highway": 4, "dense": 5}
# GSTTACO_CONV_VH_*: the bounded-input variants (two fp16 planes, three products), numbered on behind CONV_V; a call runs one only with
# the WINO_SPLIT_H form and a promised bound (ConvCall.x_absmax)
CONV_VH = {"WINO4_S": 32, "WINO2_S": 33}
CONV_V_NAMES = {v: k for k, v in CONV_V.items()}
CONV_V_NAMES.update({v: k + "_H" for k, v in CONV_VH.items()})
# GSTTACO_CONV_FORM_*: the weight forms gsttaco_debug_conv_prepare builds
CONV_FORM = {"FP32": 1, "BF16": 2, "WINO2": 4, "WINO4": 8, "WINO_SPLIT": 16, "GEMM_SPLIT": 32, "WINO_SPLIT_H": 64}


class ConvDesc(ctypes.Structure):
    _fields_ = [("taps", ctypes.c_int32), ("cin", ctypes.c_int32), ("n", ctypes.c_int32), ("ldw", ctypes.c_int32),
                ("forms", ctypes.c_int32)]


class ConvCall(ctypes.Structure):
    _fields_ = [("forms", ctypes.c_int32), ("B", ctypes.c_int32), ("T", ctypes.c_int32), ("pad_before", ctypes.c_int32),
                ("act", ctypes.c_int32), ("ldo", ctypes.c_int64),
                ("pool2", ctypes.c_int32), ("x_bf16", ctypes.c_int32), ("out_bf16", ctypes.c_int32), ("wino_x3", ctypes.c_int32),
                ("wino_min_wgs", ctypes.c_int32),
                ("conv2d", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("Wo", ctypes.c_int32), ("kw", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("pad_h", ctypes.c_int32), ("pad_w", ctypes.c_int32),
                ("x_absmax", ctypes.c_float),       # (in what was the padding in front of xb: size and offsets unchanged)
                ("xb", ctypes.c_int64)]

_I32A = ctypes.c_int32 * MAX_LAYERS


class Config(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32), ("device", ctypes.c_int32),
        ("mel_dim", ctypes.c_int32), ("step_reduction", ctypes.c_int32), ("max_step", ctypes.c_int32),
        ("vocab", ctypes.c_int32), ("emb", ctypes.c_int32), ("n_enc_conv", ctypes.c_int32),
        ("enc_filters", _I32A), ("enc_kernels", _I32A), ("enc_rnn", ctypes.c_int32),
        ("n_prenet", ctypes.c_int32), ("prenet", _I32A), ("prenet_rate", ctypes.c_float),
        ("n_dec_rnn", ctypes.c_int32), ("dec_rnn", _I32A),
        ("att_type", ctypes.c_int32), ("att_size", ctypes.c_int32), ("sigmoid_noise", ctypes.c_float),
        ("loc_filters", ctypes.c_int32), ("loc_kernel", ctypes.c_int32), ("lsa_cumulate", ctypes.c_int32),
        ("lsa_smoothing", ctypes.c_int32),
        ("n_post", ctypes.c_int32), ("post_filters", _I32A), ("post_kernels", _I32A), ("post_tanh", ctypes.c_int32),
        ("gst_use", ctypes.c_int32), ("n_ref_conv", ctypes.c_int32),
        ("ref_filters", _I32A), ("ref_kernels", _I32A), ("ref_strides", _I32A),
        ("ref_rnn", ctypes.c_int32), ("ref_dense", ctypes.c_int32), ("n_tokens", ctypes.c_int32),
        ("token_emb", ctypes.c_int32), ("heads", ctypes.c_int32), ("gst_att", ctypes.c_int32),
        ("voc_use", ctypes.c_int32), ("spec_dim", ctypes.c_int32), ("bank_count", ctypes.c_int32),
        ("bank_filters", ctypes.c_int32), ("n_voc_proj", ctypes.c_int32), ("voc_proj_filters", _I32A),
        ("voc_proj_kernels", _I32A), ("highway_count", ctypes.c_int32), ("highway_size", ctypes.c_int32),
        ("voc_rnn", ctypes.c_int32),
        ("sample_rate", ctypes.c_int32), ("frame_length", ctypes.c_int32), ("frame_shift", ctypes.c_int32),
        ("max_abs_mel", ctypes.c_float), ("max_wav_samples", ctypes.c_int32),
        ("mixed_precision", ctypes.c_int32),
        ("max_batch", ctypes.c_int32), ("max_tokens", ctypes.c_int32), ("max_ref_frames", ctypes.c_int32),
    ]


class MelganConfig(ctypes.Structure):
    _fields_ = [("mel_dim", ctypes.c_int32), ("base", ctypes.c_int32), ("n_ratios", ctypes.c_int32), ("ratios", _I32A),
                ("n_res", ctypes.c_int32), ("slope", ctypes.c_float), ("max_batch", ctypes.c_int32), ("max_frames", ctypes.c_int32)]


class WaveglowConfig(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in ("mel_dim", "hop", "win", "n_group", "n_flows", "n_early_every", "n_early_size",
                                                    "n_layers", "n_channels", "kernel", "max_batch", "max_frames")]


class HifiganConfig(ctypes.Structure):
    _fields_ = [("mel_dim", ctypes.c_int32), ("initial", ctypes.c_int32), ("n_rates", ctypes.c_int32), ("rates", _I32A),
                ("resblock", ctypes.c_int32), ("n_kernels", ctypes.c_int32), ("kernels", _I32A), ("n_dilations", _I32A),
                ("dilations", (ctypes.c_int32 * HIFIGAN_MAX_DILATIONS) * MAX_LAYERS),
                ("slope", ctypes.c_float), ("out_slope", ctypes.c_float), ("max_batch", ctypes.c_int32), ("max_frames", ctypes.c_int32)]


class GstTacoError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("gsttaco error {}: {}".format(code, message))
        self.code = code


_lib = None


def load_library(path=None):
    """dlopen the C-ABI library; fails loudly if it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # GSTTACO_LIB: an alternative build of the same ABI (A/B timing of two builds on one GPU box; tools/ab.sh)
    p = path or os.environ.get("GSTTACO_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(
            "{} not found: build the HIP extension first (python -m gst_tacotron_amd.build). "
            "There is no CPU fallback for the hot path.".format(p))
    lib = ctypes.CDLL(p)
    vp, i32, u64, f32p = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_float)
    lib.gsttaco_abi_version.restype = ctypes.c_int
    lib.gsttaco_create.argtypes = [ctypes.POINTER(Config), ctypes.POINTER(vp)]
    lib.gsttaco_destroy.argtypes = [vp]
    lib.gsttaco_destroy.restype = None
    lib.gsttaco_last_error.argtypes = [vp]
    lib.gsttaco_last_error.restype = ctypes.c_char_p
    lib.gsttaco_num_weights.argtypes = [vp]
    lib.gsttaco_weight_info.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_char_p),
                                        ctypes.POINTER(ctypes.c_int64 * 4), ctypes.POINTER(ctypes.c_int)]
    lib.gsttaco_load_weight.argtypes = [vp, ctypes.c_char_p, f32p, ctypes.POINTER(ctypes.c_int64), i32]
    lib.gsttaco_finalize_weights.argtypes = [vp]
    lib.gsttaco_encode.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.gsttaco_gst.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.gsttaco_gst_ex.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.gsttaco_style_compose.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.gsttaco_inference_step_styled.argtypes = [vp, vp, vp, vp, vp, vp, u64, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.gsttaco_decode.argtypes = [vp, vp, vp, vp, vp, vp, u64, i32, i32, i32, vp, vp, vp, vp]
    lib.gsttaco_decode_forced.argtypes = [vp, vp, vp, vp, vp, vp, u64, i32, i32, vp, i32, vp, vp, vp, vp]
    lib.gsttaco_inference_step_forced.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u64, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.gsttaco_forced_durations.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
    lib.gsttaco_fill_randomness.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    lib.gsttaco_utterance_report.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.gsttaco_losses.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]
    lib.gsttaco_mel_dtw.argtypes = [vp, vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.gsttaco_mel_dtw.restype = ctypes.c_int
    i32p = ctypes.POINTER(ctypes.c_int32)       # (host arrays)
    lib.gsttaco_resample.argtypes = [vp, vp, i32p, i32p, i32, i32, i32, vp, i32, i32p, vp]
    lib.gsttaco_resample.restype = ctypes.c_int
    f32 = ctypes.c_float
    lib.gsttaco_pitch.argtypes = [vp, vp, vp, i32, i32, f32, f32, f32, f32, i32, vp, vp, vp, i32, vp]
    lib.gsttaco_pitch.restype = ctypes.c_int
    lib.gsttaco_pitch_errors.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, i32, f32, vp, vp, vp]
    lib.gsttaco_pitch_errors.restype = ctypes.c_int
    lib.gsttaco_style_affinities.argtypes = [vp, vp, i32, i32, ctypes.c_int64, f32, vp, vp, vp, vp]
    lib.gsttaco_style_affinities.restype = ctypes.c_int
    lib.gsttaco_style_map.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, f32, i32, i32, f32, f32, f32, vp, vp]
    lib.gsttaco_style_map.restype = ctypes.c_int
    # the three vocoders: five signatures in common, then each one's own
    for prefix, config in (("melgan", MelganConfig), ("waveglow", WaveglowConfig), ("hifigan", HifiganConfig)):
        sig = {"configure": [vp, ctypes.POINTER(config)], "num_weights": [vp], "finalize": [vp], "plan": [vp, ctypes.POINTER(ctypes.c_int32)],
               "weight_info": [vp, i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64 * 4), ctypes.POINTER(ctypes.c_int)],
               "load_weight": [vp, ctypes.c_char_p, f32p, ctypes.POINTER(ctypes.c_int64), i32]}
        for name, argtypes in sig.items():
            fn = getattr(lib, "gsttaco_{}_{}".format(prefix, name))
            fn.argtypes, fn.restype = argtypes, ctypes.c_int
    for name, argtypes in (("melgan", [vp, vp, vp, i32, i32, vp, vp, i32, vp]), ("melgan_debug_stage", [vp, i32, vp, vp, i32, i32, vp, i32, vp]),
                           ("waveglow_noise", [vp, vp, i32, i32, vp, vp]), ("waveglow", [vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, i32, vp]),
                           ("waveglow_debug_stage", [vp, i32, vp, vp, i32, i32, f32, vp, vp, vp, i32, vp]),
                           ("hifigan", [vp, vp, vp, i32, i32, vp, vp, i32, vp]), ("hifigan_debug_stage", [vp, i32, vp, vp, i32, i32, vp, i32, vp]),
                           ("hifigan_set_operands", [vp, i32]), ("hifigan_debug_buffer", [vp, i32, vp, ctypes.c_int64, i32, vp])):
        fn = getattr(lib, "gsttaco_" + name)
        fn.argtypes, fn.restype = argtypes, ctypes.c_int
    lib.gsttaco_postnet.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.gsttaco_vocoder.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.gsttaco_inference_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.gsttaco_mel_frontend.argtypes = [vp, vp, vp, i32, i32, ctypes.c_float, vp, vp, i32, vp]
    lib.gsttaco_feature_frontend.argtypes = [vp, vp, vp, i32, i32, ctypes.c_float, vp, vp, vp, i32, vp]
    lib.gsttaco_mel_basis.argtypes = [vp, f32p]
    lib.gsttaco_griffin_lim.argtypes = [vp, vp, vp, i32, i32, i32, ctypes.c_float, ctypes.c_float, vp, u64, vp, vp, i32, vp]
    lib.gsttaco_set_profiling.argtypes = [vp, i32]
    lib.gsttaco_get_profile.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
    lib.gsttaco_lstm_launch_bytes.argtypes = [vp, i32, i32]
    lib.gsttaco_lstm_launch_bytes.restype = ctypes.c_int64
    lib.gsttaco_debug_stamps.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.gsttaco_debug_stamps.restype = ctypes.c_int
    lib.gsttaco_decode_plan.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_int32)]
    lib.gsttaco_decode_plan.restype = ctypes.c_int
    lib.gsttaco_debug_randomness.argtypes = [vp, vp, vp, i32, i32, i32]
    lib.gsttaco_debug_randomness.restype = ctypes.c_int
    lib.gsttaco_set_graph_policy.argtypes = [vp, i32, i32]
    lib.gsttaco_set_graph_policy.restype = ctypes.c_int
    lib.gsttaco_graph_cache_size.argtypes = [vp]
    lib.gsttaco_graph_cache_size.restype = ctypes.c_int
    lib.gsttaco_debug_handoff_error.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    lib.gsttaco_debug_handoff_error.restype = ctypes.c_int
    lib.gsttaco_debug_raise_handoff_error.argtypes = [vp, ctypes.c_uint32]
    lib.gsttaco_debug_raise_handoff_error.restype = ctypes.c_int
    lib.gsttaco_debug_counters.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.gsttaco_debug_counters.restype = ctypes.c_int
    lib.gsttaco_synchronize.argtypes = [vp, vp]
    lib.gsttaco_synchronize.restype = ctypes.c_int
    lib.gsttaco_debug_conv_prepare.argtypes = [vp, ctypes.POINTER(ConvDesc), f32p, f32p, f32p, ctypes.POINTER(ctypes.c_int)]
    lib.gsttaco_debug_conv_prepare.restype = ctypes.c_int
    lib.gsttaco_debug_conv_run.argtypes = [vp, i32, ctypes.POINTER(ConvCall), vp, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int), vp]
    lib.gsttaco_debug_conv_run.restype = ctypes.c_int
    if hasattr(lib, "gsttaco_postnet_variants"):       # (an older build of the same ABI given through GSTTACO_LIB, for A/B, has neither)
        lib.gsttaco_postnet_variants.argtypes = [vp, i32, i32, ctypes.POINTER(ctypes.c_int32)]
        lib.gsttaco_postnet_variants.restype = ctypes.c_int
        lib.gsttaco_debug_wino_h_planes.argtypes = [ctypes.POINTER(ctypes.c_double), i32, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_uint16),
                                                    ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        lib.gsttaco_debug_wino_h_planes.restype = ctypes.c_int
    if hasattr(lib, "gsttaco_encoder_variants"):       # (likewise)
        lib.gsttaco_encoder_variants.argtypes = [vp, i32, i32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        lib.gsttaco_encoder_variants.restype = ctypes.c_int
        lib.gsttaco_vocoder_variants.argtypes = [vp, i32, i32, i32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        lib.gsttaco_vocoder_variants.restype = ctypes.c_int
    if hasattr(lib, "gsttaco_decode_plan_fields"):     # (likewise)
        lib.gsttaco_decode_plan_fields.argtypes = [vp, i32, i32, i32, ctypes.POINTER(ctypes.c_int32)]
        lib.gsttaco_decode_plan_fields.restype = ctypes.c_int
    for fn in ("gsttaco_create", "gsttaco_num_weights", "gsttaco_weight_info", "gsttaco_load_weight",
               "gsttaco_finalize_weights", "gsttaco_encode", "gsttaco_gst", "gsttaco_decode", "gsttaco_postnet", "gsttaco_vocoder",
               "gsttaco_inference_step", "gsttaco_set_profiling", "gsttaco_get_profile", "gsttaco_mel_frontend",
               "gsttaco_mel_basis", "gsttaco_griffin_lim", "gsttaco_gst_ex", "gsttaco_style_compose", "gsttaco_inference_step_styled",
               "gsttaco_decode_forced", "gsttaco_inference_step_forced", "gsttaco_forced_durations",
               "gsttaco_fill_randomness", "gsttaco_utterance_report", "gsttaco_losses", "gsttaco_feature_frontend"):
        getattr(lib, fn).restype = ctypes.c_int
    if path is None:
        _lib = lib
    return lib


def make_config(hp, vocab=None, device=0, max_batch=32, max_tokens=256, max_ref_frames=1025, max_wav_seconds=0.0):
    d = Dims(hp, vocab)
    c = Config()
    c.abi_version, c.device = ABI_VERSION, device
    c.mel_dim, c.step_reduction, c.max_step = d.mel, d.r, d.max_step
    c.vocab, c.emb, c.n_enc_conv = d.vocab, d.emb, len(d.enc_filters)
    # (post_filters: Decoder.Conv.Filters plus the postnet's fixed last layer)
    for field, n in (("Encoder.Conv.Filters", len(d.enc_filters)), ("Decoder.Conv.Filters (+ 1)", len(d.post_filters)),
                     ("Decoder.Prenet.Size", len(d.prenet)), ("Decoder.RNN.Size", len(d.dec_rnn))):
        if n > MAX_LAYERS:
            raise ValueError("too many layers for the C-ABI config: {} has {} (max {})".format(field, n, MAX_LAYERS))
    for i, (f, k) in enumerate(zip(d.enc_filters, d.enc_kernels)):
        c.enc_filters[i], c.enc_kernels[i] = f, k
    c.enc_rnn = d.enc_rnn
    c.n_prenet = len(d.prenet)
    for i, s in enumerate(d.prenet):
        c.prenet[i] = s
    c.prenet_rate = d.prenet_rate
    c.n_dec_rnn = len(d.dec_rnn)
    for i, s in enumerate(d.dec_rnn):
        c.dec_rnn[i] = s
    c.att_type, c.att_size, c.sigmoid_noise = ATT_CODES[d.att_type], d.att, d.sigmoid_noise
    c.loc_filters, c.loc_kernel = d.loc_filters, d.loc_kernel
    c.lsa_cumulate, c.lsa_smoothing = int(d.lsa_cumulate), int(d.lsa_smoothing)
    c.n_post = len(d.post_filters)
    for i, (f, k) in enumerate(zip(d.post_filters, d.post_kernels)):
        c.post_filters[i], c.post_kernels[i] = f, k
    c.post_tanh = d.post_tanh
    c.gst_use = int(d.gst)
    if d.gst:
        if len(d.ref_filters) > MAX_LAYERS:
            raise ValueError("too many reference-encoder layers")
        c.n_ref_conv = len(d.ref_filters)
        for i, (f, k, s) in enumerate(zip(d.ref_filters, d.ref_kernels, d.ref_strides)):
            c.ref_filters[i], c.ref_kernels[i], c.ref_strides[i] = f, k, s
        c.ref_rnn, c.ref_dense, c.n_tokens = d.ref_rnn, d.ref_dense, d.n_tokens
        c.token_emb, c.heads, c.gst_att = d.token_emb, d.heads, d.gst_att
    c.spec_dim = d.spec
    if d.audio:
        c.sample_rate, c.frame_length, c.frame_shift, c.max_abs_mel = d.sample_rate, d.frame_length, d.frame_shift, d.max_abs_mel
        c.max_wav_samples = int(max_wav_seconds * d.sample_rate)
    elif max_wav_seconds:
        raise ValueError("Hyper_Parameters has no complete Sound section for the audio entry points")
    c.voc_use = int(d.vocoder)
    if d.vocoder:
        if len(d.voc_proj_filters) > MAX_LAYERS:
            raise ValueError("too many vocoder projection layers")
        c.bank_count, c.bank_filters = d.bank_count, d.bank_filters
        c.n_voc_proj = len(d.voc_proj_filters)
        for i, (f, k) in enumerate(zip(d.voc_proj_filters, d.voc_proj_kernels)):
            c.voc_proj_filters[i], c.voc_proj_kernels[i] = f, k
        c.highway_count, c.highway_size, c.voc_rnn = d.highway_count, d.highway_size, d.voc_rnn
    c.mixed_precision = int(bool(hp.get("Use_Mixed_Precision", False)))
    c.max_batch, c.max_tokens, c.max_ref_frames = max_batch, max_tokens, max_ref_frames
    return c


class Context:
    """RAII wrapper around gsttaco_ctx."""

    def __init__(self, hp, vocab=None, device=0, max_batch=32, max_tokens=256, max_ref_frames=1025, lib=None,
                 max_wav_seconds=0.0):
        self.lib = lib or load_library()
        self.cfg = make_config(hp, vocab, device, max_batch, max_tokens, max_ref_frames, max_wav_seconds)
        self.handle = ctypes.c_void_p()
        rc = self.lib.gsttaco_create(ctypes.byref(self.cfg), ctypes.byref(self.handle))
        if rc != 0:
            raise GstTacoError(rc, self.lib.gsttaco_last_error(None).decode())

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.gsttaco_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            raise GstTacoError(rc, self.lib.gsttaco_last_error(self.handle).decode())

    def manifest(self):
        out = {}
        n = self.lib.gsttaco_num_weights(self.handle)
        for i in range(n):
            name, shape, nd = ctypes.c_char_p(), (ctypes.c_int64 * 4)(), ctypes.c_int()
            self.check(self.lib.gsttaco_weight_info(self.handle, i, ctypes.byref(name), ctypes.byref(shape), ctypes.byref(nd)))
            out[name.value.decode()] = tuple(shape[k] for k in range(nd.value))
        return out

    def load_weights(self, weights):
        for name in self.manifest():
            if name not in weights:
                raise KeyError("missing weight '{}'".format(name))
            a = np.asarray(weights[name], dtype=np.float32, order="C")
            if not a.flags["C_CONTIGUOUS"]:
                a = a.copy()
            shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
            self.check(self.lib.gsttaco_load_weight(
                self.handle, name.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), shape, a.ndim))

    def finalize(self):
        self.check(self.lib.gsttaco_finalize_weights(self.handle))

    # ---- what the three vocoders' bindings share; ``prefix`` is "melgan", "waveglow" or "hifigan"
    def _voc_fn(self, prefix, name):
        return getattr(self.lib, "gsttaco_{}_{}".format(prefix, name))

    def _voc_manifest(self, prefix):
        out = {}
        for i in range(self._voc_fn(prefix, "num_weights")(self.handle)):
            name, shape, nd = ctypes.c_char_p(), (ctypes.c_int64 * 4)(), ctypes.c_int()
            self.check(self._voc_fn(prefix, "weight_info")(self.handle, i, ctypes.byref(name), ctypes.byref(shape), ctypes.byref(nd)))
            out[name.value.decode()] = tuple(shape[k] for k in range(nd.value))
        return out

    def _voc_load_weight(self, prefix, name, array):
        a = np.ascontiguousarray(np.asarray(array, dtype=np.float32))
        shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
        self.check(self._voc_fn(prefix, "load_weight")(self.handle, name.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), shape, a.ndim))

    def _voc_load_weights(self, prefix, weights):
        for name in self._voc_manifest(prefix):
            if name not in weights:
                raise KeyError("missing weight '{}'".format(name))
            self._voc_load_weight(prefix, name, weights[name])

    def _voc_finalize(self, prefix):
        self.check(self._voc_fn(prefix, "finalize")(self.handle))

    def _voc_plan(self, prefix, ints, stride, fields, kinds):
        """(the plan's two leading numbers, [one dict of ``fields`` per launch, ``kind`` as a name of ``kinds``])"""
        f = (ctypes.c_int32 * ints)()
        self.check(self._voc_fn(prefix, "plan")(self.handle, f))
        stages = []
        for i in range(f[0]):
            row = dict(zip(fields, f[3 + stride * i: 3 + stride * (i + 1)]))
            row["kind"] = kinds[row["kind"]]
            stages.append(row)
        return int(f[1]), int(f[2]), stages

    # ---- the neural vocoder (gsttaco_melgan_*): one per context
    def melgan_configure(self, cfg, max_batch, max_frames):
        """``cfg``: a melgan.MelGANConfig (or anything with its fields)."""
        m = MelganConfig()
        m.mel_dim, m.base, m.n_res, m.slope = int(cfg.mel_dim), int(cfg.base), int(cfg.n_res), float(cfg.slope)
        if len(cfg.ratios) > MAX_LAYERS:
            raise ValueError("at most {} upsampling ratios".format(MAX_LAYERS))
        m.n_ratios = len(cfg.ratios)
        for i, r in enumerate(cfg.ratios):
            m.ratios[i] = int(r)
        m.max_batch, m.max_frames = int(max_batch), int(max_frames)
        self.check(self.lib.gsttaco_melgan_configure(self.handle, ctypes.byref(m)))

    def melgan_manifest(self):
        return self._voc_manifest("melgan")

    def melgan_load_weight(self, name, array):
        self._voc_load_weight("melgan", name, array)

    def melgan_load_weights(self, weights):
        self._voc_load_weights("melgan", weights)

    def melgan_finalize(self):
        self._voc_finalize("melgan")

    def melgan_plan(self):
        """(min_frames, hop, [one dict of MELGAN_PLAN_FIELDS per launch, ``kind`` as a name of MELGAN_KINDS])."""
        return self._voc_plan("melgan", MELGAN_PLAN_INTS, 6, MELGAN_PLAN_FIELDS, MELGAN_KINDS)

    # ---- the flow vocoder (gsttaco_waveglow_*): one per context
    def waveglow_configure(self, cfg, max_batch, max_frames):
        """``cfg``: a waveglow.WaveGlowConfig (or anything with its fields)."""
        m = WaveglowConfig()
        for name in ("mel_dim", "hop", "win", "n_group", "n_flows", "n_early_every", "n_early_size", "n_layers", "n_channels", "kernel"):
            setattr(m, name, int(getattr(cfg, name)))
        m.max_batch, m.max_frames = int(max_batch), int(max_frames)
        self.check(self.lib.gsttaco_waveglow_configure(self.handle, ctypes.byref(m)))

    def waveglow_manifest(self):
        return self._voc_manifest("waveglow")

    def waveglow_load_weight(self, name, array):
        self._voc_load_weight("waveglow", name, array)

    def waveglow_load_weights(self, weights):
        self._voc_load_weights("waveglow", weights)

    def waveglow_finalize(self):
        self._voc_finalize("waveglow")

    def waveglow_plan(self):
        """(hop, n_group, [one dict of WAVEGLOW_PLAN_FIELDS per launch, ``kind`` as a name of WAVEGLOW_KINDS])."""
        return self._voc_plan("waveglow", WAVEGLOW_PLAN_INTS, 6, WAVEGLOW_PLAN_FIELDS, WAVEGLOW_KINDS)

    # ---- the HiFi-GAN vocoder (gsttaco_hifigan_*): one per context
    def hifigan_configure(self, cfg, max_batch, max_frames):
        """``cfg``: a hifigan.HiFiGANConfig (or anything with its fields)."""
        m = HifiganConfig()
        m.mel_dim, m.initial, m.resblock = int(cfg.mel_dim), int(cfg.initial), int(cfg.resblock)
        m.slope, m.out_slope = float(cfg.slope), float(cfg.out_slope)
        if len(cfg.rates) > MAX_LAYERS:
            raise ValueError("at most {} upsampling rates".format(MAX_LAYERS))
        if len(cfg.kernels) > MAX_LAYERS:
            raise ValueError("at most {} residual kernels".format(MAX_LAYERS))
        if len(cfg.dilations) != len(cfg.kernels):
            raise ValueError("one dilation list per residual kernel")
        m.n_rates, m.n_kernels = len(cfg.rates), len(cfg.kernels)
        for i, r in enumerate(cfg.rates):
            m.rates[i] = int(r)
        for j, (k, dils) in enumerate(zip(cfg.kernels, cfg.dilations)):
            m.kernels[j], m.n_dilations[j] = int(k), len(dils)
            for n, d in enumerate(dils[:HIFIGAN_MAX_DILATIONS]):
                m.dilations[j][n] = int(d)
        m.max_batch, m.max_frames = int(max_batch), int(max_frames)
        self.check(self.lib.gsttaco_hifigan_configure(self.handle, ctypes.byref(m)))

    def hifigan_manifest(self):
        return self._voc_manifest("hifigan")

    def hifigan_load_weight(self, name, array):
        self._voc_load_weight("hifigan", name, array)

    def hifigan_load_weights(self, weights):
        self._voc_load_weights("hifigan", weights)

    def hifigan_set_operands(self, operands):
        """``operands``: a name of HIFIGAN_OPERANDS ("float32", "bfloat16", "float16") or its number; between configure and finalize."""
        self.check(self.lib.gsttaco_hifigan_set_operands(self.handle, int(HIFIGAN_OPERANDS.get(operands, operands))))

    def hifigan_finalize(self):
        self._voc_finalize("hifigan")

    def hifigan_debug_buffer(self, buffer, tensor, write, stream=None):
        """Test support: copies the float32 device ``tensor`` into (``write``) or out of the start of workspace buffer ``buffer`` (0 .. 3
        or a name of HIFIGAN_BUFFERS) on ``stream`` (a raw stream handle; None: the null stream)."""
        k = HIFIGAN_BUFFERS.index(buffer) if isinstance(buffer, str) else int(buffer)
        self.check(self.lib.gsttaco_hifigan_debug_buffer(self.handle, k, ctypes.c_void_p(tensor.data_ptr()), int(tensor.numel()),
                                                         1 if write else 0, stream))

    def hifigan_plan(self):
        """(min_frames, hop, [one dict of HIFIGAN_PLAN_FIELDS per launch, ``kind`` as a name of HIFIGAN_KINDS])."""
        return self._voc_plan("hifigan", HIFIGAN_PLAN_INTS, 8, HIFIGAN_PLAN_FIELDS, HIFIGAN_KINDS)
