"""CPU checks of the neural vocoder: tests/melgan_cases.py's float64 restatement against a second, independent one built from
torch's own modules in the public generator's layer order (which pins the restatement, the weight-norm folding, both weight layouts
and the row-length rule at once), the admission of every case, and the host surface: symbols, manifests, refusals of
gsttaco_melgan_configure straight through the C ABI, the optional hparams section, the loader, and the model's refusal to use a
vocoder that was not loaded."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import melgan_cases as M
from gst_tacotron_amd import capi, hparams, melgan, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- 1. torch's own modules
def _torch_generator(cfg, weights, seed):
    """The public generator's ``nn.Sequential`` (weight-normalised layers, residual blocks as block + shortcut) in float64, carrying
    ``weights``: every v is the plain weight in torch's layout times a random positive factor per slice of its first axis, g the
    plain weight's norm over the other axes, so that g v / |v| is the plain weight again."""
    import torch
    from torch import nn

    class ResnetBlock(nn.Module):
        def __init__(self, dim, dilation):
            super().__init__()
            self.block = nn.Sequential(nn.LeakyReLU(cfg.slope), nn.ReflectionPad1d(dilation), wn(nn.Conv1d(dim, dim, 3, dilation=dilation)),
                                       nn.LeakyReLU(cfg.slope), wn(nn.Conv1d(dim, dim, 1)))
            self.shortcut = wn(nn.Conv1d(dim, dim, 1))

        def forward(self, x):
            return self.shortcut(x) + self.block(x)

    def wn(layer):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return nn.utils.weight_norm(layer)

    rng = np.random.default_rng(seed)

    def fill(layer, kernel, bias, transposed=False):
        k = np.asarray(weights[kernel], dtype=np.float64)
        if transposed:                  # [k, cin, cout] -> [cin, cout, k]
            w = k.transpose(1, 2, 0)
        else:                           # [taps * cin, cout] -> [cout, cin, taps]
            cout, cin = layer.weight_v.shape[0], layer.weight_v.shape[1]
            w = k.reshape(-1, cin, cout).transpose(2, 1, 0)
        assert tuple(w.shape) == tuple(layer.weight_v.shape), (kernel, w.shape, layer.weight_v.shape)
        norm = np.sqrt((w * w).reshape(w.shape[0], -1).sum(axis=1)).reshape(-1, 1, 1)
        with torch.no_grad():
            layer.weight_v.copy_(torch.from_numpy(w * rng.uniform(0.5, 2.0, norm.shape)))
            layer.weight_g.copy_(torch.from_numpy(norm))
            layer.bias.copy_(torch.from_numpy(np.asarray(weights[bias], dtype=np.float64)))

    ch = cfg.channels()
    layers = [nn.ReflectionPad1d(3), wn(nn.Conv1d(cfg.mel_dim, ch[0], 7))]
    fills = [(layers[1], "melgan/in/kernel", "melgan/in/bias", False)]
    for i, r in enumerate(cfg.ratios):
        up = wn(nn.ConvTranspose1d(ch[i], ch[i + 1], 2 * r, stride=r, padding=r // 2 + r % 2, output_padding=r % 2))
        layers += [nn.LeakyReLU(cfg.slope), up]
        fills.append((up, f"melgan/up{i}/kernel", f"melgan/up{i}/bias", True))
        for j in range(cfg.n_res):
            blk = ResnetBlock(ch[i + 1], 3 ** j)
            layers.append(blk)
            p = f"melgan/up{i}/res{j}/"
            fills += [(blk.block[2], p + "conv3/kernel", p + "conv3/bias", False), (blk.block[4], p + "conv1/kernel", p + "conv1/bias", False),
                      (blk.shortcut, p + "shortcut/kernel", p + "shortcut/bias", False)]
    out = wn(nn.Conv1d(cfg.base, 1, 7))
    layers += [nn.LeakyReLU(cfg.slope), nn.ReflectionPad1d(3), out, nn.Tanh()]
    fills.append((out, "melgan/out/kernel", "melgan/out/bias", False))

    class Generator(nn.Module):
        def __init__(self):
            super().__init__()
            self.model = nn.Sequential(*layers)

    g = Generator().double()
    for f in fills:
        fill(*f)
    return g


@pytest.mark.parametrize("name", M.NAMES)
def test_the_restatement_equals_torchs_own_modules_row_by_row(name):
    import torch
    c = M.CASES[name]
    g = _torch_generator(c.cfg, c.weights, seed=c.seed)
    sd = g.state_dict()
    assert any(k.endswith("weight_g") for k in sd) and any(k.endswith("weight_v") for k in sd)
    loaded = melgan.from_state_dict(sd)
    assert list(loaded) == list(melgan.manifest(c.cfg)) and melgan.infer_config(loaded) == c.cfg
    got, lengths = M.melgan_reference(c.cfg, {k: v.astype(np.float64) for k, v in _fold64(sd, c.cfg).items()}, c.mel, c.frames_array)
    worst = 0.0
    for b, n in enumerate(c.frames):
        if n < c.cfg.min_frames:
            assert lengths[b] == 0 and not got[b].any()
            continue
        with torch.no_grad():
            want = g.model(torch.from_numpy(c.mel[b, :n].astype(np.float64).T[None]))[0, 0].numpy()
        assert lengths[b] == n * c.cfg.hop == want.shape[0]
        worst = max(worst, float(np.abs(got[b, :lengths[b]] - want).max()))
        assert not got[b, lengths[b]:].any()
    print(name, "largest difference from torch's modules", worst)
    assert worst <= 1e-12
    # and through the float32 arrays the loader returns: the case's own weights come back to float32 rounding
    for k, v in loaded.items():
        assert v.dtype == np.float32 and np.abs(v.astype(np.float64) - c.weights[k]).max() <= 2.0 ** -22 * max(1.0, np.abs(c.weights[k]).max())


def _fold64(sd, cfg):
    """from_state_dict's arrays without their rounding to float32, which alone is 1e-8: the comparison to 1e-12 is of the layouts
    and the folding."""
    return melgan.from_state_dict(sd, dtype=np.float64)


def test_fold_weight_norm_is_torchs_dim0_rule_in_both_layouts():
    import torch
    rng = np.random.default_rng(0)
    for shape, transposed in (((6, 4, 3), False), ((6, 3, 8), True)):
        v, g = rng.normal(size=shape), rng.uniform(0.5, 2.0, (shape[0], 1, 1))
        want = torch._weight_norm(torch.from_numpy(v), torch.from_numpy(g), 0).numpy()
        assert np.abs(melgan.fold_weight_norm(g, v, transposed=transposed) - want).max() <= 1e-15


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
    assert np.array_equal(lengths, [n * c.cfg.hop if n >= c.cfg.min_frames else 0 for n in c.frames])


def test_the_table_reaches_the_edges_it_names():
    c = M.CASES
    assert c["tiny"].frames == (9, 5, 6) and c["odd_channels"].cfg.channels() == [12, 6, 3]
    e = c["min_rows"].cfg
    assert e.min_frames == 5 and c["min_rows"].frames == (5, 4, 0) and c["dilation_edge"].frames == (5, 6)
    assert 3 ** (e.n_res - 1) == 9 and e.min_frames * e.ratios[0] == 10
    t = c["tiles"]
    assert t.cfg.ratios == [8, 8, 2, 2] and t.cfg.mel_dim == 80 and t.cfg.base == 8
    tiles = M.plan_tiles(t.cfg)
    assert len(tiles) == 2 + 4 * (1 + 3) and {k for k, *_ in tiles} == {"in", "up", "res", "out"}
    for _, _, tile, _, rate in tiles:           # every boundary a frame count reaches is in, with its neighbours
        for m in (1, 2):
            if (m * tile) % rate == 0:
                assert {m * tile // rate - 1, m * tile // rate, m * tile // rate + 1} - {0} <= set(t.frames)
    assert {63, 64, 65, 127, 128, 129} <= set(t.frames) and min(t.frames) < t.cfg.min_frames
    assert c["full_size"].cfg == melgan.MelGANConfig() and c["full_size"].frames == (12, 7) and melgan.MelGANConfig().hop == 256
    h = c["hot"]
    assert set(np.unique(np.abs(h.mel))) == {np.float32(M.MAX_ABS_MEL)}


def test_the_hot_case_runs_on_the_leaky_branch():
    """Most pre-activations in front of a LeakyReLU are negative: measured on the first stage's input of the restatement."""
    c = M.CASES["hot"]
    w = {k: v.astype(np.float64) for k, v in c.weights.items()}
    x = c.mel[0, :c.frames[0]].astype(np.float64)
    h = M._conv(M._reflect(x, 3), w["melgan/in/kernel"], w["melgan/in/bias"], 7, 1)
    assert (h < 0).mean() > 0.5


def test_float32_restatement_runs_in_float32():
    c = M.CASES["tiny"]
    wav, _ = M.reference("tiny", "float32")
    assert wav.dtype == np.float32 and M.melgan_row(c.cfg, c.weights, c.mel[0].astype(np.float32)).dtype == np.float32


# ---------------------------------------------------------------------------------------------------- 3. the host surface
NEW_SYMBOLS = ("gsttaco_melgan_configure", "gsttaco_melgan_num_weights", "gsttaco_melgan_weight_info", "gsttaco_melgan_load_weight",
               "gsttaco_melgan_finalize", "gsttaco_melgan", "gsttaco_melgan_plan", "gsttaco_melgan_debug_stage")


def test_header_library_and_binding_agree_and_the_abi_is_still_14():
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    lib = capi.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert hasattr(lib, s) and s in capi.EXPORTED_SYMBOLS
    assert "#define GSTTACO_ABI_VERSION 14" in header and lib.gsttaco_abi_version() == 14 == capi.ABI_VERSION
    assert "typedef struct gsttaco_melgan_config" in header
    assert capi.MELGAN_PLAN_INTS == 3 + 6 * 74 and "#define GSTTACO_MELGAN_PLAN_INTS (3 + 6 * 74)" in header


def _ctx():
    return capi.Context(synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4)


def test_the_models_manifest_is_untouched_and_the_vocoder_has_its_own():
    from gst_tacotron_amd import weights
    ctx = _ctx()
    try:
        before = ctx.manifest()
        assert list(before) == list(weights.manifest(synthetic.tiny_hp())) and ctx.melgan_manifest() == {}
        cfg = M.CASES["odd_channels"].cfg
        ctx.melgan_configure(cfg, 2, 16)
        assert ctx.manifest() == before and ctx.lib.gsttaco_num_weights(ctx.handle) == len(before)
        assert ctx.melgan_manifest() == melgan.manifest(cfg) and not any(k.startswith("melgan") for k in before)
        min_frames, hop, stages = ctx.melgan_plan()
        assert (min_frames, hop) == (cfg.min_frames, cfg.hop)
        assert [(s["kind"], s["channels"], s["tile"], s["form"], s["rate"]) for s in stages] == M.plan_tiles(cfg)
        assert all(0 < s["lds"] <= 160 * 1024 for s in stages)
        # loads: an unknown name and a wrong shape are refused without a device, and so is a run before finalize
        with pytest.raises(capi.GstTacoError) as e:
            ctx.melgan_load_weight("melgan/in/nothing", np.zeros((1,), np.float32))
        assert e.value.code == -4 and "unknown" in str(e.value)
        with pytest.raises(capi.GstTacoError) as e:
            ctx.melgan_load_weight("melgan/in/kernel", np.zeros((7 * cfg.mel_dim + 1, 12), np.float32))
        assert e.value.code == -4 and "shape" in str(e.value)
        assert ctx.lib.gsttaco_melgan(ctx.handle, None, None, 1, 8, None, None, 8 * cfg.hop, None) == -4
        with pytest.raises(capi.GstTacoError) as e:         # one vocoder per context
            ctx.melgan_configure(cfg, 2, 16)
        assert e.value.code == -1
    finally:
        ctx.close()


@pytest.mark.parametrize("why, kwargs, text", [
    ("odd ratio", dict(ratios=[8, 3]), "odd"),
    ("ratio below 2", dict(ratios=[8, 0]), "even"),
    ("mel_dim", dict(mel_dim=0), "at least 1"),
    ("base", dict(base=0), "at least 1"),
    ("n_res", dict(n_res=0), "at least 1"),
    ("no ratios", dict(ratios=[]), "ratios"),
    ("lds: channels", dict(base=64), "LDS"),
    ("lds: halo", dict(n_res=7), "LDS"),
])
def test_configure_refusals_come_through_the_c_abi_without_a_gpu(why, kwargs, text):
    ctx = _ctx()
    try:
        with pytest.raises(capi.GstTacoError) as e:
            ctx.melgan_configure(melgan.MelGANConfig(**kwargs), 2, 16)
        assert e.value.code == -1 and text in str(e.value), (why, str(e.value))
        assert ctx.melgan_manifest() == {}
        ctx.melgan_configure(melgan.MelGANConfig(), 2, 16)          # the refusal left the context configurable
        for bad in ((0, 16), (2, 0)):
            other = _ctx()
            try:
                with pytest.raises(capi.GstTacoError):
                    other.melgan_configure(melgan.MelGANConfig(), *bad)
            finally:
                other.close()
    finally:
        ctx.close()


def test_more_than_eight_ratios_are_refused():
    ctx = _ctx()
    try:
        m = capi.MelganConfig()
        m.mel_dim, m.base, m.n_res, m.slope, m.max_batch, m.max_frames, m.n_ratios = 80, 1, 1, 0.2, 1, 8, 9
        for i in range(8):
            m.ratios[i] = 2
        assert ctx.lib.gsttaco_melgan_configure(ctx.handle, ctypes.byref(m)) == -1
        with pytest.raises(ValueError):
            ctx.melgan_configure(melgan.MelGANConfig(ratios=[2] * 9), 1, 8)
    finally:
        ctx.close()


def test_the_hparams_section_is_optional_and_its_ratios_must_make_the_frame_shift():
    hp = hparams.load_hp()
    assert "Vocoder_MelGAN" not in hp and melgan.from_hp(hp) is None
    hp["Vocoder_MelGAN"] = {"Base_Filters": 32, "Upsample_Ratios": [8, 8, 2, 2], "Residual_Layers": 3, "Checkpoint_Path": None}
    assert hp["Sound"]["Frame_Shift"] == 256
    assert melgan.from_hp(hparams.load_hp(hp)) == melgan.MelGANConfig()
    hp["Vocoder_MelGAN"]["Upsample_Ratios"] = [8, 8, 2]
    with pytest.raises(ValueError, match="Frame_Shift"):
        hparams.load_hp(hp)
    tiny = synthetic.tiny_hp()
    tiny["Vocoder_MelGAN"] = {"Base_Filters": 4, "Upsample_Ratios": [4, 2, 2], "Residual_Layers": 2}
    assert melgan.from_hp(hparams.load_hp(tiny)) == melgan.MelGANConfig(mel_dim=16, base=4, ratios=[4, 2, 2], n_res=2)


def test_from_state_dict_takes_weight_norm_pairs_and_plain_weights(tmp_path):
    import torch
    c = M.CASES["tiny"]
    sd = _torch_generator(c.cfg, c.weights, seed=3).state_dict()
    a = melgan.from_state_dict(sd)
    plain = {}
    for k, v in sd.items():
        if k.endswith("weight_g"):
            plain[k[:-2]] = torch._weight_norm(sd[k[:-1] + "v"], v, 0)
        elif not k.endswith("weight_v"):
            plain[k] = v
    b = melgan.from_state_dict(plain)
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    path = str(tmp_path / "generator.pt")
    torch.save(sd, path)
    d = melgan.load(path)
    assert all(np.array_equal(a[k], d[k]) for k in a)
    with pytest.raises(ValueError):
        melgan.from_state_dict({k: v for k, v in list(sd.items())[:6]})


def test_synthetic_weights_are_seeded_and_match_the_manifest():
    cfg = melgan.MelGANConfig()
    a, b = melgan.synthetic_weights(cfg, seed=4), melgan.synthetic_weights(cfg, seed=4)
    melgan.check_weights(cfg, a)
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    assert a["melgan/up0/kernel"].shape == (16, 512, 256) and a["melgan/up3/res2/conv3/kernel"].shape == (96, 32)
    assert cfg.min_frames == 4 and melgan.MelGANConfig(n_res=5).min_frames == 11


def test_inference_with_the_vocoder_but_without_its_weights_raises():
    from gst_tacotron_amd.model import GST_Tacotron
    m = GST_Tacotron(hyper_parameters=synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4, max_wav_seconds=0.0)
    try:
        with pytest.raises(capi.GstTacoError, match="Load_Neural_Vocoder"):
            m.Inference(["Hi."], export=True, vocoder="melgan")
        with pytest.raises(capi.GstTacoError, match="Load_Neural_Vocoder"):
            m.Neural_Vocoder(np.zeros((1, 8, 16), np.float32))
        with pytest.raises(ValueError):
            m.Inference(["Hi."], vocoder="wavenet")
    finally:
        m.ctx.close()
