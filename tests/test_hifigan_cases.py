"""CPU checks of the HiFi-GAN vocoder: tests/hifigan_cases.py's float64 restatement against a second, independent one built from
torch's own modules as the public ``Generator`` (which pins the restatement, the weight-norm folding, both weight layouts, the
separate output slope and the row-length rule at once), the admission of every case, and the host surface: symbols, manifests,
refusals of gsttaco_hifigan_configure straight through the C ABI, the optional hparams section, the loader in its three weight
spellings, and the model's refusal to use a vocoder that was not loaded."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import hifigan_cases as M
from gst_tacotron_amd import capi, hifigan, hparams, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- 1. torch's own modules
def _torch_generator(cfg, weights, seed):
    """The public ``Generator`` (weight-normalised ``conv_pre``, ``ups``, ``resblocks``, ``conv_post``; ``F.leaky_relu`` at its
    default in front of ``conv_post``) in float64, carrying ``weights``: every v is the plain weight in torch's layout times a random
    positive factor per slice of its first axis, g the plain weight's norm over the other axes, so that g v / |v| is the plain
    weight again."""
    import torch
    import torch.nn.functional as F
    from torch import nn

    def wn(layer):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return nn.utils.weight_norm(layer)

    class ResBlock1(nn.Module):
        def __init__(self, ch, k, dils):
            super().__init__()
            self.convs1 = nn.ModuleList([wn(nn.Conv1d(ch, ch, k, 1, dilation=d, padding=(k * d - d) // 2)) for d in dils])
            self.convs2 = nn.ModuleList([wn(nn.Conv1d(ch, ch, k, 1, dilation=1, padding=(k - 1) // 2)) for _ in dils])

        def forward(self, x):
            for c1, c2 in zip(self.convs1, self.convs2):
                xt = c2(F.leaky_relu(c1(F.leaky_relu(x, cfg.slope)), cfg.slope))
                x = xt + x
            return x

    class ResBlock2(nn.Module):
        def __init__(self, ch, k, dils):
            super().__init__()
            self.convs = nn.ModuleList([wn(nn.Conv1d(ch, ch, k, 1, dilation=d, padding=(k * d - d) // 2)) for d in dils])

        def forward(self, x):
            for c in self.convs:
                x = c(F.leaky_relu(x, cfg.slope)) + x
            return x

    class Generator(nn.Module):
        def __init__(self):
            super().__init__()
            ch = cfg.channels()
            self.conv_pre = wn(nn.Conv1d(cfg.mel_dim, ch[0], 7, 1, padding=3))
            self.ups = nn.ModuleList([wn(nn.ConvTranspose1d(ch[i], ch[i + 1], 2 * u, u, padding=(2 * u - u) // 2))
                                      for i, u in enumerate(cfg.rates)])
            block = ResBlock1 if cfg.resblock == 1 else ResBlock2
            self.resblocks = nn.ModuleList([block(ch[i + 1], k, d) for i in range(len(cfg.rates)) for k, d in zip(cfg.kernels, cfg.dilations)])
            self.conv_post = wn(nn.Conv1d(ch[-1], 1, 7, 1, padding=3))

        def forward(self, x):
            n_k = len(cfg.kernels)
            x = self.conv_pre(x)
            for i in range(len(cfg.rates)):
                x = self.ups[i](F.leaky_relu(x, cfg.slope))
                xs = None
                for j in range(n_k):
                    y = self.resblocks[i * n_k + j](x)
                    xs = y if xs is None else xs + y
                x = xs / n_k
            x = F.leaky_relu(x)                 # the default slope, 0.01: the contract's out_slope
            return torch.tanh(self.conv_post(x))

    rng = np.random.default_rng(seed)

    def fill(layer, prefix, transposed=False):
        k = np.asarray(weights[prefix + "/kernel"], dtype=np.float64)
        if transposed:                  # [k, cin, cout] -> [cin, cout, k]
            w = k.transpose(1, 2, 0)
        else:                           # [taps * cin, cout] -> [cout, cin, taps]
            cout, cin = layer.weight_v.shape[0], layer.weight_v.shape[1]
            w = k.reshape(-1, cin, cout).transpose(2, 1, 0)
        assert tuple(w.shape) == tuple(layer.weight_v.shape), (prefix, w.shape, layer.weight_v.shape)
        norm = np.sqrt((w * w).reshape(w.shape[0], -1).sum(axis=1)).reshape(-1, 1, 1)
        with torch.no_grad():
            layer.weight_v.copy_(torch.from_numpy(w * rng.uniform(0.5, 2.0, norm.shape)))
            layer.weight_g.copy_(torch.from_numpy(norm))
            layer.bias.copy_(torch.from_numpy(np.asarray(weights[prefix + "/bias"], dtype=np.float64)))

    g = Generator().double()
    fill(g.conv_pre, "hifigan/in")
    n_k = len(cfg.kernels)
    for i in range(len(cfg.rates)):
        fill(g.ups[i], f"hifigan/up{i}", transposed=True)
        for j in range(n_k):
            blk = g.resblocks[i * n_k + j]
            for m in range(len(cfg.dilations[j])):
                p = f"hifigan/up{i}/res{j}/unit{m}/"
                if cfg.resblock == 1:
                    fill(blk.convs1[m], p + "conv1")
                    fill(blk.convs2[m], p + "conv2")
                else:
                    fill(blk.convs[m], p + "conv1")
    fill(g.conv_post, "hifigan/out")
    return g


def _spellings(sd):
    """The state_dict as it is (weight_g / weight_v), after remove_weight_norm (plain weight), and as torch's newer parametrization
    names it (parametrizations.weight.original0 = g, original1 = v)."""
    import torch
    plain, param = {}, {}
    for k, v in sd.items():
        if k.endswith(".weight_g"):
            plain[k[:-2]] = torch._weight_norm(sd[k[:-1] + "v"], v, 0)
            param[k[:-len("weight_g")] + "parametrizations.weight.original0"] = v
        elif k.endswith(".weight_v"):
            param[k[:-len("weight_v")] + "parametrizations.weight.original1"] = v
        else:
            plain[k] = v
            param[k] = v
    return sd, plain, param


def test_the_newer_spelling_is_what_torch_writes():
    import torch
    conv = torch.nn.utils.parametrizations.weight_norm(torch.nn.Conv1d(3, 4, 5))
    keys = set(conv.state_dict())
    assert keys == {"bias", "parametrizations.weight.original0", "parametrizations.weight.original1"}
    assert tuple(conv.state_dict()["parametrizations.weight.original0"].shape) == (4, 1, 1)         # g


@pytest.mark.parametrize("name", M.NAMES)
def test_the_restatement_equals_torchs_own_modules_row_by_row(name):
    import torch
    c = M.CASES[name]
    g = _torch_generator(c.cfg, c.weights, seed=c.seed)
    sd = g.state_dict()
    assert any(k.endswith("weight_g") for k in sd) and any(k.endswith("weight_v") for k in sd)
    assert {k.split(".")[0] for k in sd} == {"conv_pre", "ups", "resblocks", "conv_post"}
    fold64 = hifigan.from_state_dict(sd, dtype=np.float64)      # without the rounding to float32, which alone is 1e-8
    got, lengths = M.hifigan_reference(c.cfg, fold64, c.mel, c.frames_array)
    worst = 0.0
    for b, n in enumerate(c.frames):
        if n < 1:
            assert lengths[b] == 0 and not got[b].any()
            continue
        with torch.no_grad():
            want = g(torch.from_numpy(c.mel[b, :n].astype(np.float64).T[None]))[0, 0].numpy()
        assert lengths[b] == n * c.cfg.hop == want.shape[0]
        worst = max(worst, float(np.abs(got[b, :lengths[b]] - want).max()))
        assert not got[b, lengths[b]:].any()
    print(name, "largest difference from torch's modules", worst)
    assert worst <= 1e-12
    # and through the float32 arrays the loader returns, in all three spellings: the case's own weights come back to float32 rounding
    for spelled in _spellings(sd):
        for wrap in (spelled, {"generator": spelled}):
            loaded = hifigan.from_state_dict(wrap)
            assert list(loaded) == list(hifigan.manifest(c.cfg))
            assert hifigan.infer_config(loaded, dilations=c.cfg.dilations) == c.cfg
            for k, v in loaded.items():
                assert v.dtype == np.float32
                assert np.abs(v.astype(np.float64) - c.weights[k]).max() <= 2.0 ** -22 * max(1.0, np.abs(c.weights[k]).max()), k


def test_the_output_slope_is_its_own_field():
    """The trap: with out_slope = slope the waveform differs from the public generator's by far more than rounding."""
    c = M.CASES["tiny"]
    assert c.cfg.out_slope == 0.01 and c.cfg.slope == 0.1 and hifigan.HiFiGANConfig().out_slope == 0.01
    import dataclasses
    wrong = dataclasses.replace(c.cfg, out_slope=c.cfg.slope)
    a = M.hifigan_row(c.cfg, c.weights, c.mel[0].astype(np.float64))
    b = M.hifigan_row(wrong, c.weights, c.mel[0].astype(np.float64))
    assert np.abs(a - b).max() > 1e-3


def test_fold_weight_norm_is_torchs_dim0_rule_in_both_layouts():
    import torch
    rng = np.random.default_rng(0)
    for shape in ((6, 4, 3), (6, 3, 8)):
        v, g = rng.normal(size=shape), rng.uniform(0.5, 2.0, (shape[0], 1, 1))
        want = torch._weight_norm(torch.from_numpy(v), torch.from_numpy(g), 0).numpy()
        assert np.abs(hifigan.fold_weight_norm(g, v) - want).max() <= 1e-15


# ---------------------------------------------------------------------------------------------------- 2. admission
@pytest.mark.parametrize("name", M.NAMES)
def test_every_case_is_admitted(name):
    c = M.CASES[name]
    wav, lengths = M.reference(name)
    live = np.concatenate([wav[b, :lengths[b]] for b in range(len(c.frames))])
    peak, saturated, e32 = float(np.abs(live).max()), float((np.abs(live) > 0.999).mean()), M.e32(name)
    print(name, "peak", peak, "share above 0.999", saturated, "e32", e32)
    assert peak >= 0.1
    assert saturated < 0.5
    if c.hot:
        assert saturated > 0
    assert e32 <= M.E32_MAX
    assert np.isfinite(wav).all() and np.abs(wav).max() <= 1.0
    assert np.array_equal(lengths, [min(n, c.T) * c.cfg.hop for n in c.frames])


def test_the_length_rule():
    c = M.CASES["tiny"]
    wav, lengths = M.hifigan_reference(c.cfg, c.weights, c.mel, np.array([100, 1, 2, 0]))       # frames above T count as T
    assert list(lengths) == [9 * c.cfg.hop, c.cfg.hop, 2 * c.cfg.hop, 0] and c.cfg.min_frames == 1
    assert np.array_equal(wav[0], M.reference("tiny")[0][0]) and not wav[3].any() and wav[1, :c.cfg.hop].any() and not wav[1, c.cfg.hop:].any()


def test_the_table_reaches_the_edges_it_names():
    c = M.CASES
    t = c["tiny"].cfg
    assert c["tiny"].frames == (9, 1, 2, 0) and t.resblock == 1 and len(t.kernels) == 2 and t.rates == [2, 2]
    assert len(t.dilations[0]) != len(t.dilations[1])
    # at one frame the rows are 1, 2 and 4 samples: the input conv's halo (3) and every dilated conv's (4, 5, 6) reach beyond the row
    # on both sides at every stage, and every closing conv's taps (3, 5) span more than the first stage's row
    assert c["tiny"].frames[1] * t.hop == 4 and all((k - 1) // 2 * d >= 4 for k, dils in zip(t.kernels, t.dilations) for d in dils)
    assert all(k > t.rates[0] for k in t.kernels)
    o = c["odd_channels"].cfg
    assert o.resblock == 2 and o.mel_dim == 7 and o.channels() == [12, 6, 3] and o.kernels == [3, 5, 11] and o.rates == [4, 2]
    assert 1 in [len(d) for d in o.dilations]
    assert len(c["one_kernel"].cfg.kernels) == 1 and c["one_kernel"].cfg.resblock == 1
    assert len(c["one_kernel_v3"].cfg.kernels) == 1 and c["one_kernel_v3"].cfg.resblock == 2
    h = c["halo"]
    assert h.cfg.kernels[0] == 11 and h.cfg.dilations[0] == [5] and h.cfg.resblock == 1
    first = [n * h.cfg.rates[0] for n in h.frames]
    assert first == [24, 26, 28, 30, 32]                # below and above the conv's 25, and below, at and above the unit's 30
    tl = c["tiles"]
    assert tl.cfg.rates == [8, 8, 2, 2] and tl.cfg.mel_dim == 80 and 32 <= tl.cfg.initial <= 64
    tiles = M.plan_tiles(tl.cfg)
    assert len(tiles) == 2 + 4 * (1 + 3 * 3 * 2) and {k for k, *_ in tiles} == {"in", "up", "conv", "out"}
    for *_, tile, _, rate in tiles:             # every boundary a frame count reaches is in, with its neighbours
        for m in (1, 2):
            if (m * tile) % rate == 0:
                assert {m * tile // rate - 1, m * tile // rate, m * tile // rate + 1} - {0} <= set(tl.frames)
    assert {255, 256, 257, 511, 512, 513, 31, 32, 33, 1, 2, 3} <= set(tl.frames)
    assert c["v1"].cfg == hifigan.HiFiGANConfig.v1() == hifigan.HiFiGANConfig() and c["v1"].frames == (12, 7)
    assert c["v3"].cfg == hifigan.HiFiGANConfig.v3() and c["v3"].frames == (12, 7)
    for cfg in (hifigan.HiFiGANConfig.v1(), hifigan.HiFiGANConfig.v2(), hifigan.HiFiGANConfig.v3()):
        assert cfg.hop == 256 and cfg.min_frames == 1
    assert hifigan.HiFiGANConfig.v2().initial == 128 and hifigan.HiFiGANConfig.v3().dilations == [[1, 2], [2, 6], [3, 12]]
    assert set(np.unique(np.abs(c["hot"].mel))) == {np.float32(M.MAX_ABS_MEL)}


def test_the_hot_case_runs_on_the_leaky_branch():
    """Most pre-activations in front of a LeakyReLU are negative: measured on the first stage's input of the restatement."""
    c = M.CASES["hot"]
    w = {k: v.astype(np.float64) for k, v in c.weights.items()}
    x = c.mel[0, :c.frames[0]].astype(np.float64)
    h = M._conv(x, w["hifigan/in/kernel"], w["hifigan/in/bias"], 7, 1)
    assert (h < 0).mean() > 0.5


def test_float32_restatement_runs_in_float32():
    c = M.CASES["tiny"]
    wav, _ = M.reference("tiny", "float32")
    assert wav.dtype == np.float32 and M.hifigan_row(c.cfg, c.weights, c.mel[0].astype(np.float32)).dtype == np.float32


# ---------------------------------------------------------------------------------------------------- 3. the host surface
NEW_SYMBOLS = ("gsttaco_hifigan_configure", "gsttaco_hifigan_num_weights", "gsttaco_hifigan_weight_info", "gsttaco_hifigan_load_weight",
               "gsttaco_hifigan_finalize", "gsttaco_hifigan", "gsttaco_hifigan_plan", "gsttaco_hifigan_debug_stage")


def test_header_library_and_binding_agree_and_the_abi_is_still_14():
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    lib = capi.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert hasattr(lib, s) and s in capi.EXPORTED_SYMBOLS
    assert "#define GSTTACO_ABI_VERSION 14" in header and lib.gsttaco_abi_version() == 14 == capi.ABI_VERSION
    assert "typedef struct gsttaco_hifigan_config" in header and "float out_slope;" in header
    assert capi.HIFIGAN_PLAN_INTS == 3 + 8 * 522 and "#define GSTTACO_HIFIGAN_PLAN_INTS (3 + 8 * 522)" in header
    assert "#define GSTTACO_HIFIGAN_MAX_DILATIONS 4" in header and capi.HIFIGAN_MAX_DILATIONS == 4
    assert "hifigan.hip" in __import__("gst_tacotron_amd.build", fromlist=["SOURCES"]).SOURCES


def _ctx():
    return capi.Context(synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4)


@pytest.mark.parametrize("name", ["odd_channels", "tiny", "v1", "v3"])
def test_the_models_manifest_is_untouched_and_the_vocoder_has_its_own(name):
    from gst_tacotron_amd import weights
    ctx = _ctx()
    try:
        before = ctx.manifest()
        assert list(before) == list(weights.manifest(synthetic.tiny_hp())) and ctx.hifigan_manifest() == {}
        cfg = M.CASES[name].cfg
        ctx.hifigan_configure(cfg, 2, 16)
        assert ctx.manifest() == before and ctx.lib.gsttaco_num_weights(ctx.handle) == len(before)
        assert list(ctx.hifigan_manifest().items()) == list(hifigan.manifest(cfg).items())
        assert not any(k.startswith("hifigan") for k in before)
        assert ctx.melgan_manifest() == {} and ctx.waveglow_manifest() == {}
        min_frames, hop, stages = ctx.hifigan_plan()
        assert (min_frames, hop) == (1, cfg.hop)
        assert [(s["kind"], s["channels"], s["taps"], s["dilation"], s["tile"], s["form"], s["rate"]) for s in stages] == M.plan_tiles(cfg)
        assert all(0 < s["lds"] <= 160 * 1024 for s in stages)
        # loads: an unknown name and a wrong shape are refused without a device, and so is a run before finalize
        with pytest.raises(capi.GstTacoError) as e:
            ctx.hifigan_load_weight("hifigan/in/nothing", np.zeros((1,), np.float32))
        assert e.value.code == -4 and "unknown" in str(e.value)
        with pytest.raises(capi.GstTacoError) as e:
            ctx.hifigan_load_weight("hifigan/in/kernel", np.zeros((7 * cfg.mel_dim + 1, cfg.initial), np.float32))
        assert e.value.code == -4 and "shape" in str(e.value)
        assert ctx.lib.gsttaco_hifigan(ctx.handle, None, None, 1, 8, None, None, 8 * cfg.hop, None) == -4
        with pytest.raises(capi.GstTacoError) as e:         # one HiFi-GAN per context
            ctx.hifigan_configure(cfg, 2, 16)
        assert e.value.code == -1
        ctx.melgan_configure(__import__("gst_tacotron_amd.melgan", fromlist=["MelGANConfig"]).MelGANConfig(), 2, 16)    # beside the others
    finally:
        ctx.close()


@pytest.mark.parametrize("why, kwargs, text", [
    ("odd rate", dict(rates=[8, 3]), "rates"),
    ("rate below 2", dict(rates=[8, 0]), "rates"),
    ("mel_dim", dict(mel_dim=0), "mel_dim"),
    ("initial", dict(initial=0), "initial"),
    ("initial not halved four times", dict(initial=24), "initial"),
    ("no rates", dict(rates=[]), "n_rates"),
    ("resblock", dict(resblock=3), "resblock"),
    ("no kernels", dict(kernels=[], dilations=[]), "n_kernels"),
    ("even kernel", dict(kernels=[3, 4, 11]), "kernels"),
    ("kernel above 11", dict(kernels=[3, 7, 13]), "kernels"),
    ("no dilations", dict(dilations=[[1, 3, 5], [], [1, 3, 5]]), "n_dilations"),
    ("five dilations", dict(dilations=[[1, 3, 5], [1, 2, 3, 4, 5], [1, 3, 5]]), "n_dilations"),
    ("dilation 0", dict(dilations=[[1, 3, 5], [1, 0, 5], [1, 3, 5]]), "dilations"),
    ("slope", dict(slope=2.0), "slope"),
    ("out_slope", dict(out_slope=-0.5), "out_slope"),
    ("lds: channels", dict(initial=4096), "LDS"),
    ("lds: halo", dict(dilations=[[1, 3, 5], [1, 3, 5], [1, 3, 1000]]), "LDS"),
])
def test_configure_refusals_come_through_the_c_abi_without_a_gpu(why, kwargs, text):
    ctx = _ctx()
    try:
        with pytest.raises(capi.GstTacoError) as e:
            ctx.hifigan_configure(hifigan.HiFiGANConfig(**kwargs), 2, 16)
        assert e.value.code == -1 and text in str(e.value), (why, str(e.value))
        assert ctx.hifigan_manifest() == {}
        with pytest.raises(capi.GstTacoError) as e:         # and nothing is configured: the plan is refused too
            ctx.hifigan_plan()
        assert e.value.code == -4
        ctx.hifigan_configure(hifigan.HiFiGANConfig(), 2, 16)       # the refusal left the context configurable
    finally:
        ctx.close()


def test_capacities_and_counts_above_eight_are_refused():
    for bad in ((0, 16), (2, 0)):
        ctx = _ctx()
        try:
            with pytest.raises(capi.GstTacoError) as e:
                ctx.hifigan_configure(hifigan.HiFiGANConfig(), *bad)
            assert e.value.code == -1 and "max_" in str(e.value)
        finally:
            ctx.close()
    ctx = _ctx()
    try:
        def raw(n_rates, n_kernels):
            m = capi.HifiganConfig()
            m.mel_dim, m.initial, m.resblock, m.slope, m.out_slope, m.max_batch, m.max_frames = 80, 512, 1, 0.1, 0.01, 1, 8
            m.n_rates, m.n_kernels = n_rates, n_kernels
            for i in range(8):
                m.rates[i], m.kernels[i], m.n_dilations[i], m.dilations[i][0] = 2, 3, 1, 1
            return ctx.lib.gsttaco_hifigan_configure(ctx.handle, ctypes.byref(m))
        assert raw(9, 3) == -1 and "n_rates" in ctx.lib.gsttaco_last_error(ctx.handle).decode()
        assert raw(4, 9) == -1 and "n_kernels" in ctx.lib.gsttaco_last_error(ctx.handle).decode()
        assert ctx.lib.gsttaco_hifigan_configure(ctx.handle, None) == -1
        with pytest.raises(ValueError):
            ctx.hifigan_configure(hifigan.HiFiGANConfig(rates=[2] * 9), 1, 8)
        with pytest.raises(ValueError):
            ctx.hifigan_configure(hifigan.HiFiGANConfig(kernels=[3] * 9, dilations=[[1]] * 9), 1, 8)
        with pytest.raises(ValueError):
            ctx.hifigan_configure(hifigan.HiFiGANConfig(kernels=[3, 7]), 1, 8)         # two kernels, three dilation lists
        assert raw(8, 8) == 0                   # the largest counts are accepted (initial 512 = 2 * 2^8)
    finally:
        ctx.close()


def test_the_hparams_section_is_optional_and_its_rates_must_make_the_frame_shift():
    hp = hparams.load_hp()
    assert "Vocoder_HiFiGAN" not in hp and hifigan.from_hp(hp) is None
    hp["Vocoder_HiFiGAN"] = {"Initial_Filters": 512, "Upsample_Rates": [8, 8, 2, 2], "Resblock": 1, "Resblock_Kernel_Sizes": [3, 7, 11],
                             "Resblock_Dilation_Sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]], "Checkpoint_Path": None}
    assert hp["Sound"]["Frame_Shift"] == 256
    assert hifigan.from_hp(hparams.load_hp(hp)) == hifigan.HiFiGANConfig.v1()
    hp["Vocoder_HiFiGAN"] = {}
    assert hifigan.from_hp(hparams.load_hp(hp)) == hifigan.HiFiGANConfig.v1()
    hp["Vocoder_HiFiGAN"] = {"Initial_Filters": 256, "Upsample_Rates": [8, 8, 4], "Resblock": 2, "Resblock_Kernel_Sizes": [3, 5, 7],
                             "Resblock_Dilation_Sizes": [[1, 2], [2, 6], [3, 12]]}
    assert hifigan.from_hp(hparams.load_hp(hp)) == hifigan.HiFiGANConfig.v3()
    hp["Vocoder_HiFiGAN"]["Upsample_Rates"] = [8, 8, 2]
    with pytest.raises(ValueError, match="Frame_Shift"):
        hparams.load_hp(hp)
    hp["Vocoder_HiFiGAN"]["Upsample_Rates"] = [8, 8, 4]
    hp["Vocoder_HiFiGAN"]["Resblock"] = 3
    with pytest.raises(ValueError, match="Resblock"):
        hparams.load_hp(hp)
    hp["Vocoder_HiFiGAN"]["Resblock"] = 2
    hp["Vocoder_HiFiGAN"]["Resblock_Dilation_Sizes"] = [[1, 2], [2, 6]]
    with pytest.raises(ValueError, match="Resblock_Dilation_Sizes"):
        hparams.load_hp(hp)
    tiny = synthetic.tiny_hp()
    tiny["Vocoder_HiFiGAN"] = {"Initial_Filters": 16, "Upsample_Rates": [4, 2, 2], "Resblock": 2, "Resblock_Kernel_Sizes": [3, 5],
                               "Resblock_Dilation_Sizes": [[1], [2, 3]]}
    assert hifigan.from_hp(hparams.load_hp(tiny)) == hifigan.HiFiGANConfig(mel_dim=16, initial=16, rates=[4, 2, 2], resblock=2,
                                                                          kernels=[3, 5], dilations=[[1], [2, 3]])


def test_load_reads_state_dicts_bare_or_under_generator(tmp_path):
    import torch
    c = M.CASES["tiny"]
    sd = _torch_generator(c.cfg, c.weights, seed=3).state_dict()
    a = hifigan.from_state_dict(sd)
    for tag, obj in (("bare", sd), ("wrapped", {"generator": sd, "steps": 5})):
        path = str(tmp_path / (tag + ".pt"))
        torch.save(obj, path)
        d = hifigan.load(path)
        assert list(a) == list(d) and all(np.array_equal(a[k], d[k]) for k in a)
    with pytest.raises(ValueError):
        hifigan.from_state_dict({k: v for k, v in sd.items() if not k.startswith("conv_post")})
    with pytest.raises(ValueError):
        hifigan.from_state_dict({k: v for k, v in sd.items() if not k.startswith("resblocks")})
    # the dilations are not in a state_dict: an unshipped shape must name them, a shipped one need not
    with pytest.raises(ValueError, match="dilations"):
        hifigan.infer_config(a)
    with pytest.raises(ValueError, match="dilations"):
        hifigan.infer_config(a, dilations=[[1, 2], [3, 4]])
    for cfg in (hifigan.HiFiGANConfig.v2(), hifigan.HiFiGANConfig.v3()):
        shapes = {k: np.zeros(s, np.float32) for k, s in hifigan.manifest(cfg).items()}
        assert hifigan.infer_config(shapes) == cfg


def test_synthetic_weights_are_seeded_and_match_the_manifest():
    cfg = hifigan.HiFiGANConfig.v1()
    a, b = hifigan.synthetic_weights(cfg, seed=4), hifigan.synthetic_weights(cfg, seed=4)
    hifigan.check_weights(cfg, a)
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    assert a["hifigan/up0/kernel"].shape == (16, 512, 256) and a["hifigan/up3/res2/unit2/conv2/kernel"].shape == (11 * 32, 32)
    assert a["hifigan/out/kernel"].shape == (7 * 32, 1) and len(a) == 2 * 78
    v3 = hifigan.manifest(hifigan.HiFiGANConfig.v3())
    assert "hifigan/up2/res2/unit1/conv1/kernel" in v3 and not any("conv2" in k for k in v3) and len(v3) == 2 * 23
    with pytest.raises(ValueError):
        hifigan.check_weights(hifigan.HiFiGANConfig.v2(), a)
    with pytest.raises(KeyError):
        hifigan.check_weights(cfg, {k: v for k, v in a.items() if k != "hifigan/out/bias"})


def test_inference_with_the_vocoder_but_without_its_weights_raises():
    from gst_tacotron_amd.model import GST_Tacotron
    m = GST_Tacotron(hyper_parameters=synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4, max_wav_seconds=0.0)
    try:
        with pytest.raises(capi.GstTacoError, match="Load_HiFiGAN"):
            m.Inference(["Hi."], export=True, vocoder="hifigan")
        with pytest.raises(capi.GstTacoError, match="Load_HiFiGAN"):
            m.HiFiGAN(np.zeros((1, 8, 16), np.float32))
        with pytest.raises(ValueError):
            m.Inference(["Hi."], vocoder="wavenet")
    finally:
        m.ctx.close()
