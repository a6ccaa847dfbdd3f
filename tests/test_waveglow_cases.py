"""CPU checks of the flow vocoder: every case of tests/waveglow_cases.py is admitted (finite, audible, log-scales within 4, each z
column used once, a float32 run within 2^-14 of the float64 one); the float64 restatement against torch's own ConvTranspose1d /
Conv1d / weight_norm modules composed per the contract, through ``waveglow.from_state_dict`` in both conditioning layouts; the channel
schedule; the refusals ``waveglow.py`` mirrors and the library's own at configure, which needs no GPU; folding and ``infer_config``
round trips."""
import os
import re

import numpy as np
import pytest

import waveglow_cases as M
from gst_tacotron_amd import capi, synthetic, waveglow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gsttaco_waveglow_configure", "gsttaco_waveglow_num_weights", "gsttaco_waveglow_weight_info", "gsttaco_waveglow_load_weight",
               "gsttaco_waveglow_finalize", "gsttaco_waveglow_noise", "gsttaco_waveglow", "gsttaco_waveglow_plan", "gsttaco_waveglow_debug_stage")


# ---------------------------------------------------------------------------------------------------- the cases are admitted
@pytest.mark.parametrize("name", M.NAMES)
def test_every_case_is_admitted(name):
    """Measured here (e32, max |s|, peak): tiny 5.9e-7 / 0.84 / 2.7, odd_channels 3.9e-7 / 0.62 / 2.0, dilation_edge 3.6e-7 / 0.56 / 1.9,
    early_default 1.4e-6 / 0.89 / 2.9, early_g4 2.7e-7 / 0.62 / 1.9, early_g16 5.2e-7 / 0.77 / 2.1, win_1 2.9e-7 / 0.72 / 1.8, win_2
    5.2e-7 / 0.98 / 2.7, win_8 3.6e-7 / 0.80 / 1.6, tiles 1.2e-6 / 1.17 / 3.6, full_size 4.4e-6 / 1.03 / 9.0, hot 2.9e-5 / 2.71 / 39."""
    c = M.CASES[name]
    wav, lengths, smax = M.reference(name)
    e32 = M.e32(name)
    print("waveglow case", name, "e32", e32, "max |s|", smax, "peak", np.abs(wav).max())
    assert np.isfinite(wav).all() and np.isfinite(M.reference(name, "float32")[0]).all()
    assert np.abs(wav).max() >= 0.1
    assert smax <= 4.0
    assert e32 <= M.E32_MAX
    assert np.array_equal(lengths, [max(0, min(n, c.T)) * c.cfg.hop for n in c.frames])
    for b, n in enumerate(lengths):
        assert not wav[b, n:].any()
    used = []
    b = int(np.argmax(c.frames))
    M.waveglow_row(c.cfg, c.weights, c.mel[b, :c.frames[b]].astype(np.float64), c.z[b, :c.frames[b] * c.cfg.hop], c.sigma, used=used)
    assert sorted(used) == list(range(c.cfg.n_group)) and used[:c.cfg.n_rem] == list(range(c.cfg.n_rem))


def test_the_table_reaches_the_edges_it_names():
    C = M.CASES
    assert C["tiny"].frames == (9, 1, 0, 5) and C["tiny"].T == 9
    odd = C["odd_channels"].cfg
    assert odd.n_channels % 16 and odd.spect_dim == 40 and odd.spect_dim % 16
    edge = C["dilation_edge"]
    cols = [n * edge.cfg.hop // edge.cfg.n_group for n in edge.frames]
    assert edge.cfg.n_layers == 5 and min(cols) == 2 and max(cols) == 6 and 2 ** (edge.cfg.n_layers - 1) >= 16 > max(cols)
    assert C["early_default"].cfg.flow_channels() == waveglow.WaveGlowConfig().flow_channels()
    assert C["early_g4"].cfg.flow_channels() == [4, 4, 2] and C["early_g16"].cfg.flow_channels() == [16, 16, 14, 14]
    assert [C[n].cfg.win // C[n].cfg.hop for n in ("win_1", "win_2", "win_8")] == [1, 2, 8] and C["win_8"].T == 3
    assert C["tiles"].frames == (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
    assert C["full_size"].cfg == waveglow.WaveGlowConfig() and C["full_size"].frames == (6, 3)
    hot = C["hot"]
    assert hot.sigma == 1.0 and 2.5 <= M.reference("hot")[2] <= 4.0 and hot.gain_s > waveglow.synthetic_weights.__defaults__[1]


def test_the_channel_schedule_of_the_defaults():
    cfg = waveglow.WaveGlowConfig()
    assert cfg.flow_channels() == [8] * 4 + [6] * 4 + [4] * 4 and cfg.n_rem == 4 and cfg.spect_dim == 640
    assert cfg.macs_per_sample() == 12 * 8 * ((768 + 640) * 512 + 256 * 512) / 8        # about 10 M a sample


def test_float32_restatement_runs_in_float32():
    c = M.CASES["tiny"]
    wav, _ = M.waveglow_row(c.cfg, c.weights, c.mel[0].astype(np.float32), c.z[0], c.sigma)
    assert wav.dtype == np.float32


# ---------------------------------------------------------------------------------------------------- against torch's own modules
def _torch_waveglow(cfg, layout, seed):
    """The public model's modules in float64: ``upsample``, ``WN.<k>`` (weight-normalised start / in_layers / res_skip_layers and the
    conditioning as one ``cond_layer`` or as ``cond_layers``, a plain ``end``) and ``convinv.<k>.conv``, randomly initialised."""
    import torch
    from torch import nn
    torch.manual_seed(seed)
    C, S, NL = cfg.n_channels, cfg.spect_dim, cfg.n_layers
    wn = lambda layer: nn.utils.weight_norm(layer, name="weight")

    class WN(nn.Module):
        def __init__(self, h):
            super().__init__()
            self.start = wn(nn.Conv1d(h, C, 1))
            self.in_layers = nn.ModuleList([wn(nn.Conv1d(C, 2 * C, 3, dilation=2 ** i, padding=2 ** i)) for i in range(NL)])
            self.res_skip_layers = nn.ModuleList([wn(nn.Conv1d(C, 2 * C if i < NL - 1 else C, 1)) for i in range(NL)])
            if layout == "cond_layer":
                self.cond_layer = wn(nn.Conv1d(S, 2 * C * NL, 1))
            else:
                self.cond_layers = nn.ModuleList([wn(nn.Conv1d(S, 2 * C, 1)) for _ in range(NL)])
            self.end = nn.Conv1d(C, 2 * h, 1)

        def forward(self, a0, spect):
            hid, out = self.start(a0), 0
            whole = self.cond_layer(spect) if layout == "cond_layer" else None
            for i in range(NL):
                cond = whole[:, 2 * C * i:2 * C * (i + 1)] if whole is not None else self.cond_layers[i](spect)
                acts = self.in_layers[i](hid) + cond
                rs = self.res_skip_layers[i](torch.tanh(acts[:, :C]) * torch.sigmoid(acts[:, C:]))
                if i < NL - 1:
                    hid, out = hid + rs[:, :C], out + rs[:, C:]
                else:
                    out = out + rs
            return self.end(out)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.upsample = nn.ConvTranspose1d(cfg.mel_dim, cfg.mel_dim, cfg.win, stride=cfg.hop)
            self.WN = nn.ModuleList([WN(c // 2) for c in cfg.flow_channels()])
            self.convinv = nn.ModuleList()
            for c in cfg.flow_channels():
                holder = nn.Module()
                holder.conv = nn.Conv1d(c, c, 1, bias=False)
                with torch.no_grad():
                    holder.conv.weight.copy_((torch.linalg.qr(torch.randn(c, c, dtype=torch.float64))[0] + 0.05 * torch.randn(c, c, dtype=torch.float64))[:, :, None])
                self.convinv.append(holder)

        def infer(self, mel, z, sigma):
            """mel [n, mel_dim], z [n * hop] -> wav [n * hop], composed per the contract of include/gsttaco.h"""
            G, n = cfg.n_group, mel.shape[0]
            up = self.upsample(mel.T[None])[:, :, :n * cfg.hop]                                    # the crop
            spect = up.unfold(2, G, G).permute(0, 2, 1, 3).reshape(1, -1, cfg.mel_dim * G).permute(0, 2, 1)
            zz = z.reshape(-1, G).T[None]                                                           # [1, G, L]
            chans = cfg.flow_channels()
            zcol = chans[-1]
            audio = sigma * zz[:, :zcol]
            for k in range(cfg.n_flows - 1, -1, -1):
                h = chans[k] // 2
                a0, a1 = audio[:, :h], audio[:, h:]
                o = self.WN[k](a0, spect)
                a1 = (a1 - o[:, :h]) * torch.exp(-o[:, h:])
                audio = torch.nn.functional.conv1d(torch.cat([a0, a1], 1), torch.linalg.inv(self.convinv[k].conv.weight[:, :, 0])[:, :, None])
                if k % cfg.n_early_every == 0 and k > 0:
                    audio = torch.cat([sigma * zz[:, zcol:zcol + cfg.n_early_size], audio], 1)
                    zcol += cfg.n_early_size
            return audio[0].T.reshape(-1)

    return Net().double()


@pytest.mark.parametrize("layout", ["cond_layer", "cond_layers"])
@pytest.mark.parametrize("name", ["tiny", "odd_channels", "early_g4", "win_8"])
def test_the_restatement_equals_torchs_own_modules_through_the_loader(name, layout):
    import torch
    c = M.CASES[name]
    net = _torch_waveglow(c.cfg, layout, seed=c.seed)
    sd = net.state_dict()
    assert any(k.endswith("weight_g") for k in sd) and ("WN.0.cond_layer.weight_v" in sd) == (layout == "cond_layer")
    w = waveglow.from_state_dict(sd, dtype=np.float64)
    waveglow.check_weights(c.cfg, w)
    assert waveglow.infer_config(w, hop=c.cfg.hop) == c.cfg
    worst = 0.0
    with torch.no_grad():
        for b, n in enumerate(c.frames):
            if n < 1:
                continue
            x, z = c.mel[b, :n].astype(np.float64), c.z[b, :n * c.cfg.hop].astype(np.float64)
            want = net.infer(torch.from_numpy(x), torch.from_numpy(z), c.sigma).numpy()
            got, _ = M.waveglow_row(c.cfg, w, x, z, c.sigma)
            assert np.abs(want).max() > 0.1
            worst = max(worst, float(np.abs(got - want).max()))
    assert worst <= 1e-12, worst
    # the float32 arrays the device gets are the folded ones, rounded once
    w32 = waveglow.from_state_dict(sd)
    assert all(v.dtype == np.float32 and np.array_equal(v, w[k].astype(np.float32)) for k, v in w32.items())


def test_from_state_dict_takes_plain_weights_and_load_reads_state_dicts_only(tmp_path):
    import torch
    c = M.CASES["tiny"]
    sd = _torch_waveglow(c.cfg, "cond_layer", seed=3).state_dict()
    plain = {}
    for k, v in sd.items():
        if k.endswith("weight_g"):
            plain[k[:-2]] = torch._weight_norm(sd[k[:-1] + "v"], v, 0)
        elif not k.endswith("weight_v"):
            plain[k] = v
    a, b = waveglow.from_state_dict(sd, dtype=np.float64), waveglow.from_state_dict(plain, dtype=np.float64)
    assert a.keys() == b.keys() and all(np.abs(a[k] - b[k]).max() <= 1e-15 for k in a)
    torch.save({"state_dict": sd}, tmp_path / "wg.pt")
    got = waveglow.load(str(tmp_path / "wg.pt"))
    assert all(np.array_equal(got[k], a[k].astype(np.float32)) for k in a)
    torch.save([1, 2, 3], tmp_path / "other.pt")
    with pytest.raises(ValueError, match="state_dict"):
        waveglow.load(str(tmp_path / "other.pt"))
    with pytest.raises(KeyError):
        waveglow.from_state_dict({k: v for k, v in sd.items() if not k.startswith("WN.1.start")})


def test_synthetic_weights_are_seeded_match_the_manifest_and_round_trip():
    for cfg in (M.CASES["tiny"].cfg, M.CASES["early_g16"].cfg, M.CASES["odd_channels"].cfg):
        a, b, other = waveglow.synthetic_weights(cfg, seed=4), waveglow.synthetic_weights(cfg, seed=4), waveglow.synthetic_weights(cfg, seed=5)
        assert list(a) == list(waveglow.manifest(cfg)) and all(np.array_equal(a[k], b[k]) for k in a)
        assert any(not np.array_equal(a[k], other[k]) for k in a)
        waveglow.check_weights(cfg, a)
        assert waveglow.infer_config(a, hop=cfg.hop) == cfg
        hot = waveglow.synthetic_weights(cfg, seed=4, gain_s=1.0)
        assert np.allclose(hot["waveglow/flow0/end/kernel"], 4.0 * a["waveglow/flow0/end/kernel"], rtol=1e-6)
        assert np.array_equal(hot["waveglow/flow0/layer0/in/kernel"], a["waveglow/flow0/layer0/in/kernel"])
    single = waveglow.WaveGlowConfig(n_flows=3, n_early_every=4)            # no early output at all
    assert waveglow.infer_config({k: np.zeros(s, np.float32) for k, s in waveglow.manifest(single).items()}).flow_channels() == [8, 8, 8]
    with pytest.raises(KeyError):
        waveglow.check_weights(cfg, {k: v for k, v in a.items() if k != "waveglow/up/bias"})
    with pytest.raises(ValueError, match="shape"):
        waveglow.check_weights(cfg, dict(a, **{"waveglow/up/bias": np.zeros((3,), np.float32)}))


def test_the_hparams_section_is_optional():
    hp = synthetic.tiny_hp()
    assert waveglow.from_hp(hp) is None
    hp["Vocoder_WaveGlow"] = {"Flows": 4, "Group": 4, "Early_Every": 2, "Early_Size": 2, "Layers": 3, "Channels": 32}
    cfg = waveglow.from_hp(hp)
    assert (cfg.mel_dim, cfg.hop, cfg.win) == (hp["Sound"]["Mel_Dim"], hp["Sound"]["Frame_Shift"], 4 * hp["Sound"]["Frame_Shift"])
    assert (cfg.n_flows, cfg.n_group, cfg.n_layers, cfg.n_channels, cfg.flow_channels()) == (4, 4, 3, 32, [4, 4, 2, 2])
    hp["Vocoder_WaveGlow"]["Group"] = 3
    with pytest.raises(ValueError, match="n_group"):
        waveglow.from_hp(hp)


# ---------------------------------------------------------------------------------------------------- header, library, refusals
def test_header_library_and_binding_agree_and_the_abi_is_still_14():
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    lib = capi.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert hasattr(lib, s) and s in capi.EXPORTED_SYMBOLS
    assert "#define GSTTACO_ABI_VERSION 14" in header and lib.gsttaco_abi_version() == 14 == capi.ABI_VERSION
    assert "typedef struct gsttaco_waveglow_config" in header
    assert capi.WAVEGLOW_PLAN_INTS == 3 + 6 * 354 and "#define GSTTACO_WAVEGLOW_PLAN_INTS (3 + 6 * 354)" in header
    assert 354 == 2 + waveglow.MAX_FLOWS * (waveglow.MAX_LAYERS + 1)


def _ctx():
    return capi.Context(synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4)


def test_the_models_manifest_is_untouched_and_the_flow_vocoder_has_its_own():
    ctx = _ctx()
    try:
        before = ctx.manifest()
        assert ctx.waveglow_manifest() == {}
        cfg = M.CASES["tiles"].cfg
        ctx.waveglow_configure(cfg, 2, 16)
        assert ctx.manifest() == before and ctx.melgan_manifest() == {}
        assert ctx.waveglow_manifest() == waveglow.manifest(cfg) and list(ctx.waveglow_manifest()) == list(waveglow.manifest(cfg))
        hop, G, stages = ctx.waveglow_plan()
        assert (hop, G) == (cfg.hop, cfg.n_group) and len(stages) == 2 + cfg.n_flows * (cfg.n_layers + 1)
        assert [s["kind"] for s in stages] == ["up", "flow"] + (["layer"] * cfg.n_layers + ["flow"]) * cfg.n_flows
        assert tuple(dict.fromkeys((s["tile"], s["unit"]) for s in stages)) == M.TILES_PLAN
        assert all(0 < s["lds"] <= 160 * 1024 for s in stages)
        with pytest.raises(capi.GstTacoError) as e:
            ctx.waveglow_load_weight("waveglow/up/nothing", np.zeros((1,), np.float32))
        assert e.value.code == -4 and "unknown" in str(e.value)
        with pytest.raises(capi.GstTacoError) as e:
            ctx.waveglow_load_weight("waveglow/up/bias", np.zeros((cfg.mel_dim + 1,), np.float32))
        assert e.value.code == -4 and "shape" in str(e.value)
        assert ctx.lib.gsttaco_waveglow(ctx.handle, None, None, 1, 8, 0.6, None, None, None, None, 8 * cfg.hop, None) == -4
        with pytest.raises(capi.GstTacoError) as e:         # one per context
            ctx.waveglow_configure(cfg, 2, 16)
        assert e.value.code == -1 and "already" in str(e.value)
    finally:
        ctx.close()


REFUSALS = [
    ("win % hop", dict(win=1000), "win"),
    ("hop % G", dict(hop=252, win=1008), "hop"),
    ("G % 2", dict(n_group=7, hop=252, win=1008), "n_group"),
    ("ES % 2", dict(n_early_size=1), "n_early_size"),
    ("c_k % 2", dict(n_group=6, hop=252, win=1008, n_early_size=3), "n_early_size"),
    ("n_rem < 2", dict(n_early_size=4), "n_early_size"),
    ("mel_dim", dict(mel_dim=0), "mel_dim"),
    ("hop", dict(hop=0), "hop"),
    ("win", dict(win=0), "win"),
    ("n_group", dict(n_group=0), "n_group"),
    ("n_flows", dict(n_flows=0), "n_flows"),
    ("n_early_every", dict(n_early_every=0), "n_early_every"),
    ("n_early_size", dict(n_early_size=0), "n_early_size"),
    ("n_layers", dict(n_layers=0), "n_layers"),
    ("n_channels", dict(n_channels=0), "n_channels"),
    ("NL > 10", dict(n_layers=11), "n_layers"),
    ("F > 32", dict(n_flows=33, n_early_every=64), "n_flows"),
    ("G > 16", dict(n_group=18, hop=252, win=1008), "n_group"),
    ("kernel", dict(kernel=5), "kernel"),
]


@pytest.mark.parametrize("why, kwargs, field", REFUSALS)
def test_configure_refusals_name_the_field_here_and_through_the_c_abi(why, kwargs, field):
    cfg = waveglow.WaveGlowConfig(**kwargs)
    with pytest.raises(ValueError, match=field):
        cfg.check()
    ctx = _ctx()
    try:
        with pytest.raises(capi.GstTacoError) as e:
            ctx.waveglow_configure(cfg, 2, 16)
        assert e.value.code == -1 and field in str(e.value), (why, str(e.value))
        assert ctx.waveglow_manifest() == {}
        ctx.waveglow_configure(waveglow.WaveGlowConfig(), 2, 16)            # the refusal left the context configurable
    finally:
        ctx.close()


@pytest.mark.parametrize("kwargs, caps, field", [
    (dict(n_channels=1024), (2, 16), "n_channels"),         # the gated tile alone is 64 x 1028 floats: beyond 160 KB of LDS
    (dict(), (0, 16), "max_batch"),
    (dict(), (2, 0), "max_frames"),
    (dict(), (4096, 4096), "max_batch"),                    # 2^32 samples
])
def test_the_librarys_own_refusals_at_configure(kwargs, caps, field):
    ctx = _ctx()
    try:
        with pytest.raises(capi.GstTacoError) as e:
            ctx.waveglow_configure(waveglow.WaveGlowConfig(**kwargs), *caps)
        assert e.value.code == -1 and field in str(e.value) and ("LDS" in str(e.value)) == bool(kwargs)
    finally:
        ctx.close()
