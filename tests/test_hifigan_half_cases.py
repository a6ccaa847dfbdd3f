"""CPU tests of the HiFi-GAN vocoder's 16-bit operand forms: the rounding's host statement, the restatements of
tests/hifigan_half_cases.py (admitted before tests/test_gpu_hifigan_half.py holds csrc/hifigan.hip to them), and the host surface of
gsttaco_hifigan_set_operands / gsttaco_hifigan_debug_buffer, which needs no device."""
import os
import re

import numpy as np
import pytest

import hifigan_cases as M
import hifigan_half_cases as H
from gst_tacotron_amd import capi, hifigan, hparams, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- 1. the rounding
def test_bfloat16_rounds_to_nearest_even_by_bits():
    r = lambda v: hifigan.round_operand(np.asarray(v, dtype=np.float32), "bfloat16")
    one, ulp = np.float32(1.0), np.float32(2.0 ** -7)                   # bf16 has 8 significant bits: its ulp at 1 is 2^-7
    assert r(one + ulp / 2) == one                                      # a tie goes to the even neighbour: down here,
    assert r(one + ulp + ulp / 2) == one + 2 * ulp                      # up here
    assert r(one + ulp / 2 + np.float32(2.0 ** -23)) == one + ulp       # and just above the tie, up
    assert r(-(one + ulp / 2)) == -one
    assert r(np.float32(3.3895314e38)) == np.float32(3.3895314e38)      # the largest bf16 is exact; above its half ulp: inf
    assert np.isinf(r(np.float32(3.4e38))) and np.isnan(r(np.float32("nan")))
    tiny = np.float32(2.0 ** -133)                                      # the smallest bf16 subnormal; half of it is a tie to 0
    assert r(tiny) == tiny and r(tiny / 2) == 0 and r(tiny * np.float32(0.75)) == tiny and r(np.float32(1.5) * tiny) == 2 * tiny
    assert hifigan.round_operand(np.float64(1.0) + 2.0 ** -8, "bfloat16").dtype == np.float64


def test_bfloat16_is_torchs_on_a_random_vector():
    import torch
    rng = np.random.default_rng(3)
    with np.errstate(over="ignore"):                                    # every binade, the subnormals and a few inf
        x = (rng.normal(0, 1, 200000) * 10.0 ** rng.integers(-44, 39, 200000)).astype(np.float32)
    assert np.array_equal(hifigan.round_operand(x, "bfloat16"), torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy())
    bits = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    bits = bits[~np.isnan(bits)]
    assert np.array_equal(hifigan.round_operand(bits, "bfloat16"), torch.from_numpy(bits).to(torch.bfloat16).to(torch.float32).numpy())


def test_float16_saturates_and_keeps_subnormals():
    r = lambda v: hifigan.round_operand(np.asarray(v, dtype=np.float32), "float16")
    assert np.array_equal(r([1e6, -1e6, 65504.0, 65519.0, 65520.0, np.inf, -np.inf]), [65504, -65504, 65504, 65504, 65504, 65504, -65504])
    one, ulp = np.float32(1.0), np.float32(2.0 ** -10)
    assert r(one + ulp / 2) == one and r(one + ulp + ulp / 2) == one + 2 * ulp and r(one + ulp / 2 + np.float32(2.0 ** -23)) == one + ulp
    sub = np.float32(2.0 ** -24)                                        # the smallest fp16 subnormal
    assert r(sub) == sub and r(sub / 2) == 0 and r(np.float32(1.5) * sub) == 2 * sub and r(np.float32(0.75) * sub) == sub
    assert r(np.float32(2.0 ** -14) - sub) == np.float32(2.0 ** -14) - sub        # the largest subnormal is exact
    assert np.isnan(r(np.float32("nan")))
    x = np.random.default_rng(4).normal(0, 300, 100000).astype(np.float32)
    assert np.array_equal(r(x), x.astype(np.float16).astype(np.float32))


def test_float32_is_the_identity_and_other_names_are_refused():
    x = np.random.default_rng(5).normal(0, 1, 100).astype(np.float32)
    assert hifigan.round_operand(x, "float32") is x
    for bad in ("int8", "fp16", None, 16):
        with pytest.raises(ValueError):
            hifigan.round_operand(x, bad)


# ---------------------------------------------------------------------------------------------------- 2. the restatements
@pytest.mark.parametrize("name", M.NAMES)
def test_half_row_at_float32_is_bitwise_the_fp32_restatement(name):
    c = M.CASES[name]
    for b, n in enumerate(c.frames):
        if n >= 1 and (name not in ("tiles", "v1", "v3") or b == 0):
            for dt in (np.float32, np.float64):
                x = c.mel[b, :n].astype(dt)
                assert np.array_equal(H.half_row(c.cfg, c.weights, x, "float32"), M.hifigan_row(c.cfg, c.weights, x))


@pytest.mark.parametrize("precision", H.PRECISIONS)
@pytest.mark.parametrize("name", M.NAMES)
def test_every_case_is_admitted_by_its_rounding_error(name, precision):
    """e_h = max |rounded-operand float64 run - exact float64 run|, seen: bfloat16 tiny 6.5e-3, odd_channels 6.3e-3, one_kernel 8.2e-3,
    one_kernel_v3 6.0e-3, halo 2.1e-2, tiles 5.6e-2, v1 5.4e-2, v3 4.0e-2, hot 3.7e-2; float16 7.3e-4, 1.6e-3, 2.2e-3, 1.6e-3, 2.8e-3,
    9.2e-3, 5.7e-3, 3.6e-3, 7.8e-3.  A case that strays beyond 2^-3 / 2^-6 is changed, not excused."""
    e = H.e_h(name, precision)
    print("hifigan", precision, "case", name, "e_h", e, "e32", M.e32(name))
    assert 0 < e <= H.E_H_MAX[precision]
    assert e > 100 * M.e32(name)                    # the rounding is really there, far above an fp32 chain's noise
    ref = H.reference(name, precision)
    assert np.isfinite(ref).all() and np.abs(ref).max() <= 1.0 and not ref.flags.writeable


@pytest.mark.parametrize("precision", ("float32",) + H.PRECISIONS)
@pytest.mark.parametrize("name", M.NAMES)
def test_the_launches_composed_along_the_plan_are_the_chain_exactly(name, precision):
    c = M.CASES[name]
    n = min(v for v in c.frames if v >= 1) if name in ("tiles", "v1", "v3") else max(c.frames)
    x = c.mel[c.frames.index(n), :n].astype(np.float64)
    assert np.array_equal(H.compose(c.cfg, c.weights, x, precision), H.half_row(c.cfg, c.weights, x, precision))


@pytest.mark.parametrize("name", ["tiny", "odd_channels", "v1", "v3"])
def test_the_launch_table_is_the_plans(name):
    cfg = M.CASES[name].cfg
    ls = H.launches(cfg)
    assert [(l.kind, l.cout, l.taps, l.dil) for l in ls] == [t[:4] for t in M.plan_tiles(cfg)]
    assert [l.rate_in if l.kind == "up" else l.rate_out for l in ls] == [t[6] for t in M.plan_tiles(cfg)]
    assert [l.name + leaf for l in ls for leaf in ("/kernel", "/bias")] == list(hifigan.manifest(cfg))
    assert H.ws_floats_per_frame(cfg) == max(r * M._pad16(ch) for r, ch in zip(np.cumprod([1] + list(cfg.rates)), cfg.channels()))


def test_a_launch_reference_takes_rows_of_unequal_lengths_and_an_empty_row():
    c = M.CASES["tiny"]
    ls = H.launches(c.cfg, c.weights)
    rng = np.random.default_rng(0)
    conv = next(l for l in ls if l.kind == "conv" and l.sum == H.SUM_ADD)
    lengths = [3, 0, 1]
    rows = lambda: [rng.normal(0, 1, (n * conv.rate_in, conv.cin)) for n in lengths]
    ins = {"x": rows(), "res": rows(), "sum": rows()}
    out = H.launch_reference(conv, ins, lengths, "bfloat16")
    assert [o.shape for o in out] == [(n * conv.rate_out, conv.cout) for n in lengths]
    alone = H.launch_reference(conv, {k: v[2:] for k, v in ins.items()}, lengths[2:], "bfloat16")
    assert np.array_equal(alone[0], out[2])
    assert not np.array_equal(out[0], H.launch_reference(conv, ins, lengths, "float32")[0])


# ---------------------------------------------------------------------------------------------------- 3. the host surface
NEW_SYMBOLS = ("gsttaco_hifigan_set_operands", "gsttaco_hifigan_debug_buffer")


def _ctx():
    return capi.Context(synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4)


def test_the_two_new_symbols_are_in_the_header_the_library_and_the_binding():
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    lib = capi.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert hasattr(lib, s) and s in capi.EXPORTED_SYMBOLS
    assert "#define GSTTACO_ABI_VERSION 14" in header and lib.gsttaco_abi_version() == 14 == capi.ABI_VERSION
    for name, value in capi.HIFIGAN_OPERANDS.items():
        tag = {"float32": "F32", "bfloat16": "BF16", "float16": "F16"}[name]
        assert re.search(r"#define\s+GSTTACO_HIFIGAN_%s\s+%d\b" % (tag, value), header)
    assert tuple(capi.HIFIGAN_OPERANDS) == hifigan.PRECISIONS and hasattr(capi.Context, "hifigan_set_operands")
    assert hasattr(capi.Context, "hifigan_debug_buffer") and capi.HIFIGAN_BUFFERS == ("sum", "up", "a", "b")


def test_set_operands_refuses_bad_values_and_bad_order_without_a_gpu():
    ctx = _ctx()
    try:
        err = lambda: ctx.lib.gsttaco_last_error(ctx.handle).decode()
        assert ctx.lib.gsttaco_hifigan_set_operands(None, 0) == -1
        assert ctx.lib.gsttaco_hifigan_set_operands(ctx.handle, 1) == -4 and "configure" in err()      # before configure
        assert ctx.lib.gsttaco_hifigan_set_operands(ctx.handle, 3) == -1                                 # a bad value, configured or not
        cfg = M.CASES["v1"].cfg
        ctx.hifigan_configure(cfg, 2, 16)
        fp32 = ctx.hifigan_plan()
        for bad in (3, -1, 16):
            assert ctx.lib.gsttaco_hifigan_set_operands(ctx.handle, bad) == -1 and "operands" in err()
        assert ctx.hifigan_plan() == fp32                                                                # a refusal changes nothing
        lds = lambda plan: [s["lds"] for s in plan[2]]
        rest = lambda plan: (plan[0], plan[1], [{k: v for k, v in s.items() if k != "lds"} for s in plan[2]])
        for name in ("bfloat16", "float16", 1, 2):
            ctx.hifigan_set_operands(name)
            half = ctx.hifigan_plan()
            # the fp32 plan's launches, tiles and forms; the LDS need only shrinks (the output conv, fp32 in every form, keeps its own)
            assert rest(half) == rest(fp32)
            assert all(h <= f for h, f in zip(lds(half), lds(fp32))) and lds(half)[-1] == lds(fp32)[-1]
            assert all(h < f for h, f, s in zip(lds(half), lds(fp32), fp32[2]) if s["kind"] != "out")
        ctx.hifigan_set_operands("float32")
        assert ctx.hifigan_plan() == fp32                                                                # and back
        # a debug_buffer before finalize is refused, a bad index too (the order of the two checks is not promised)
        assert ctx.lib.gsttaco_hifigan_debug_buffer(ctx.handle, 0, None, 0, 0, None) == -4 and "finalize" in err()
        assert ctx.lib.gsttaco_hifigan_debug_buffer(None, 0, None, 0, 0, None) == -1
    finally:
        ctx.close()


def test_the_16_bit_tile_is_what_the_header_says():
    """Rows of round32(C_p) + 8 sixteen-bit elements against the fp32 form's C_p + 4 floats, the same number of rows."""
    ctx = _ctx()
    try:
        cfg = M.CASES["odd_channels"].cfg           # C_p = 16: the k block of 32 pads every row
        ctx.hifigan_configure(cfg, 2, 16)
        fp32 = ctx.hifigan_plan()[2]
        ctx.hifigan_set_operands("bfloat16")
        half = ctx.hifigan_plan()[2]
        cins = [l.cin for l in H.launches(cfg)]
        for f, h, cin in zip(fp32, half, cins):
            if f["kind"] != "out":
                cp = M._pad16(cin)
                rows = f["lds"] // (4 * (cp + 4))
                assert f["lds"] == rows * 4 * (cp + 4) and h["lds"] == rows * 2 * ((cp + 31) // 32 * 32 + 8)
    finally:
        ctx.close()


def test_the_precision_argument_and_the_hparams_key():
    from gst_tacotron_amd.model import GST_Tacotron
    hp = hparams.load_hp()
    assert hifigan.precision_from_hp(hp) == "float32"
    sec = {"Initial_Filters": 512, "Upsample_Rates": [8, 8, 2, 2], "Precision": "bfloat16"}
    hp["Vocoder_HiFiGAN"] = dict(sec)
    loaded = hparams.load_hp(hp)
    assert hifigan.precision_from_hp(loaded) == "bfloat16"
    cfg = hifigan.from_hp(loaded)                                       # the key is tolerated and is no part of the network
    assert cfg == hifigan.HiFiGANConfig.v1() and not hasattr(cfg, "precision") and not hasattr(cfg, "Precision")
    hp["Vocoder_HiFiGAN"]["Precision"] = "float16"
    assert hifigan.precision_from_hp(hparams.load_hp(hp)) == "float16"
    hp["Vocoder_HiFiGAN"]["Precision"] = None
    assert hifigan.precision_from_hp(hparams.load_hp(hp)) == "float32"
    hp["Vocoder_HiFiGAN"]["Precision"] = "int8"
    with pytest.raises(ValueError, match="Precision"):
        hparams.load_hp(hp)
    with pytest.raises(ValueError, match="precision"):
        hifigan.precision_from_hp(hp)
    tiny = synthetic.tiny_hp()
    tiny["Use_Mixed_Precision"] = True                                  # the decoder's switch is not the vocoder's
    assert hifigan.precision_from_hp(tiny) == "float32"
    m = GST_Tacotron(hyper_parameters=synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4, max_wav_seconds=0.0)
    try:
        vc = hifigan.HiFiGANConfig(mel_dim=16, initial=16, rates=[4, 2, 2], resblock=1, kernels=[3, 5], dilations=[[1, 2], [3]])
        w = hifigan.synthetic_weights(vc, seed=8)
        for bad in ("int8", "half", 16):
            with pytest.raises(ValueError, match="precision"):
                m.Load_HiFiGAN(w, config=vc, precision=bad)
        assert m._hifigan is None and m._hifigan_precision is None and m.ctx.hifigan_manifest() == {}      # refused before anything was configured
    finally:
        m.ctx.close()
