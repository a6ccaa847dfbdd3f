"""GPU tests of the flow vocoder (csrc/waveglow.hip through gsttaco_waveglow): every case of tests/waveglow_cases.py with injected z
against the float64 restatement, row by row over the row's length, to K times the case's own float32-restatement error; lengths, the
zeros beyond a row and the empty rows exactly; the bitwise properties the header promises (a repeated call, a row alone, a larger
capacity, a captured graph, seeds against the noise they stand for, a noise prefix); the device's noise against a host Box-Muller;
sigma; every refusal straight through the C ABI; and Inference(export=True, vocoder="waveglow") end to end.

The measured ratios of device error to e32 stand at test_every_case_equals_the_float64_restatement_row_by_row and in DESIGN 3.5."""
import ctypes
import os

import numpy as np
import pytest

import waveglow_cases as M
from vocoder_harness import Vocoder, seeds_tensor as _seeds
from gst_tacotron_amd import capi, melgan, synthetic, waveglow
from oracle import rng_np

pytestmark = pytest.mark.gpu

# The bar is K * e32(case).  The device and the float32 restatement are fp32 chains of one depth that differ in summation order and in
# the last ulps of tanh / sigmoid / exp; K is the smallest power of two at least twice the largest measured ratio (the docstring of
# test_every_case...: 2.07, twice that is 4.14), never above 16.
K = 8
STREAM_WAVEGLOW = 0x8000            # GT_RNG_WAVEGLOW: the 4th Philox counter word of the flow vocoder's z
SEED = 0x9E3779B97F4A7C15           # a seed whose high 32 bits are set
# Box-Muller on the device's fast intrinsics against float64 on the same float32 uniforms, the maximum over the samples of
# test_the_noise_is_the_host_box_muller, measured on an MI355X.  NOISE_TOL is 4 x that (the rule of tests/test_gpu_rng.py).
NOISE_ERR_MEASURED = 8.696e-7
NOISE_TOL = 4 * NOISE_ERR_MEASURED

_VOCODERS = {}


def _Vocoder(cfg, weights, max_batch, max_frames, finalize=True):
    """A context that holds nothing but a finalized flow vocoder."""
    return Vocoder("waveglow", cfg, weights, max_batch, max_frames, finalize)


@pytest.fixture(scope="module", autouse=True)
def _close_the_contexts():
    """Every context of this module lives for the module only (the persistent decode launch of later files needs to be the process's
    one live context)."""
    yield
    for v in _VOCODERS.values():
        v.close()
    _VOCODERS.clear()


def _vocoder(name):
    """One vocoder per case configuration, sized for the case, kept for the module."""
    c = M.CASES[name]
    if name not in _VOCODERS:
        _VOCODERS[name] = _Vocoder(c.cfg, c.weights, len(c.frames), c.T)
    return _VOCODERS[name]


def _worst(wav, want, want_len, tag):
    worst = 0.0
    for b, n in enumerate(want_len):
        assert not wav[b, n:].any(), (tag, b)                   # zeros beyond the row, exactly; an empty row is all zeros
        if n:
            worst = max(worst, float(np.abs(wav[b, :n].astype(np.float64) - want[b, :n]).max()))
    return worst


# ---------------------------------------------------------------------------------------------------- 1. every case against float64
@pytest.mark.parametrize("name", M.NAMES)
def test_every_case_equals_the_float64_restatement_row_by_row(name):
    """Largest device error over the case's rows / e32(case), measured on an MI355X: tiny 0.89 (5.3e-7 / 5.9e-7), odd_channels 0.84
    (3.3e-7 / 3.9e-7), dilation_edge 0.70 (2.5e-7 / 3.6e-7), early_default 0.57 (7.9e-7 / 1.4e-6), early_g4 1.96 (5.3e-7 / 2.7e-7),
    early_g16 0.95 (5.0e-7 / 5.2e-7), win_1 1.22 (3.5e-7 / 2.9e-7), win_2 0.66 (3.4e-7 / 5.2e-7), win_8 0.70 (2.5e-7 / 3.6e-7), tiles 1.09
    (1.3e-6 / 1.2e-6), full_size 1.68 (7.4e-6 / 4.4e-6), hot 2.07 (5.9e-5 / 2.8e-5).  Twice the largest is 4.14: K = 8.  None is above 8,
    the mark at which the issue reads a ratio as a finding about the kernel."""
    c = M.CASES[name]
    want, want_len, _ = M.reference(name)
    e32 = M.e32(name)
    v = _vocoder(name)
    if name == "tiles":         # the case's rows come from the tiles the library really uses
        hop, G, stages = v.ctx.waveglow_plan()
        assert tuple(M.tile_edge_frames(stages, hop)) == c.frames
    wav, lengths = v(c.mel, c.frames_array, z=c.z, sigma=c.sigma)
    assert np.array_equal(lengths, want_len)
    assert np.isfinite(wav).all()
    worst = _worst(wav, want, want_len, name)
    print("waveglow case", name, "device error", worst, "e32", e32, "ratio", worst / e32)
    assert worst <= K * e32
    assert (want_len == 0).sum() == sum(n < 1 for n in c.frames)


# ---------------------------------------------------------------------------------------------------- 2. bitwise properties
@pytest.mark.parametrize("name", ["tiny", "tiles", "full_size"])
def test_a_call_repeats_and_a_row_in_its_batch_is_the_row_alone(name):
    c = M.CASES[name]
    v = _vocoder(name)
    hop = c.cfg.hop
    wav, lengths = v(c.mel, c.frames_array, z=c.z, sigma=c.sigma)
    again, _ = v(c.mel, c.frames_array, z=c.z, sigma=c.sigma)
    assert np.array_equal(wav, again)
    rows = [b for b, n in enumerate(c.frames) if n >= 1]
    for b in rows[:2] + rows[-3:]:
        n = c.frames[b]
        alone, alone_len = v(c.mel[b:b + 1, :n], z=c.z[b:b + 1, :n * hop], sigma=c.sigma)         # B = 1, T = its frames, no lengths
        assert alone_len[0] == lengths[b] == n * hop and np.array_equal(alone[0], wav[b, :lengths[b]]), (name, b)
    wide, _ = v(c.mel, c.frames_array, z=c.z, sigma=c.sigma, ld=c.T * hop + 37)                  # a wider wav: zeros in the extra columns
    assert np.array_equal(wide[:, :wav.shape[1]], wav) and not wide[:, wav.shape[1]:].any()


def test_a_large_call_leaves_nothing_behind_for_a_small_one():
    """Capacity 4 x 40 frames: a full-capacity call, then a small one, against the small one on a fresh context of exactly its size --
    stale workspace behind a row's end must not leak in."""
    c = M.CASES["tiles"]
    rng = np.random.default_rng(9)
    big = _Vocoder(c.cfg, c.weights, 4, 40)
    try:
        full, full_len = big(rng.uniform(-4, 4, (4, 40, c.cfg.mel_dim)), seeds=[1, 2, 3, 4])
        assert (full_len == 40 * c.cfg.hop).all() and np.abs(full).max() > 0.1
        small_mel = rng.uniform(-4, 4, (2, 9, c.cfg.mel_dim)).astype(np.float32)
        got = big(small_mel, [5, 9], seeds=[7, 8])
    finally:
        big.close()
    fresh = _Vocoder(c.cfg, c.weights, 2, 9)
    try:
        want = fresh(small_mel, [5, 9], seeds=[7, 8])
    finally:
        fresh.close()
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]) and np.abs(want[0]).max() > 0.1


def test_the_call_is_captured_in_a_graph_and_replays_bitwise():
    """No allocation and no synchronisation inside the call: it is captured on a side stream and replayed twice."""
    import torch
    c = M.CASES["tiny"]
    v = _vocoder("tiny")
    eager, eager_len = v(c.mel, c.frames_array, z=c.z, sigma=c.sigma)
    x, fr, z = torch.as_tensor(c.mel).cuda(), torch.as_tensor(c.frames_array).cuda(), torch.as_tensor(c.z).cuda()
    B, T = x.shape[:2]
    ld = T * c.cfg.hop
    wav = torch.full((B, ld), float("nan"), dtype=torch.float32, device="cuda")
    lens = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = v.raw(x, fr, B, T, c.sigma, None, z, wav, lens, ld)
    assert rc == 0
    for _ in range(2):
        wav.fill_(float("nan"))
        lens.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(wav.cpu().numpy(), eager) and np.array_equal(lens.cpu().numpy(), eager_len)


def test_seeds_are_the_noise_they_stand_for():
    """seeds= is bitwise z = gsttaco_waveglow_noise(seeds); the first n * hop samples at T = n are those at a larger T; a row's noise
    is its seed's, whatever its place in the batch; different seeds differ."""
    c = M.CASES["tiny"]
    v = _vocoder("tiny")
    hop = c.cfg.hop
    seeds = [SEED, 5, SEED, 0]
    z = v.noise(seeds, c.T)
    assert np.isfinite(z).all() and np.array_equal(z[0], z[2]) and not np.array_equal(z[0], z[1]) and not np.array_equal(z[1], z[3])
    assert np.array_equal(v.noise([5], 4)[0], z[1, :4 * hop]) and np.array_equal(v.noise([0, SEED], 2)[1], z[0, :2 * hop])
    assert not np.array_equal(v.noise([SEED & 0xFFFFFFFF], c.T)[0], z[0])                      # the key's high word counts
    by_seed, lens = v(c.mel, c.frames_array, seeds=seeds, sigma=c.sigma)
    by_z, lens_z = v(c.mel, c.frames_array, z=z, sigma=c.sigma)
    assert np.array_equal(by_seed, by_z) and np.array_equal(lens, lens_z) and np.abs(by_seed).max() > 0.1
    other, _ = v(c.mel, c.frames_array, seeds=[1, 2, 3, 4], sigma=c.sigma)
    assert not np.array_equal(other[0], by_seed[0])


def test_nan_beyond_a_row_reaches_no_sample():
    """What lies beyond a row's frames (mel) and samples (z) may be NaN -- in Inference(..., vocoder=) the decoder's free run past the
    stop token is what sits there: a bound taken as a product passes a finite filler and fails this.  The wav and the lengths are
    bitwise those of the plain call."""
    c = M.CASES["tiny"]
    v = _vocoder("tiny")
    hop = c.cfg.hop
    wav, lengths = v(c.mel, c.frames_array, z=c.z, sigma=c.sigma)
    mel, z = c.mel.copy(), c.z.copy()
    for b, n in enumerate(c.frames):
        mel[b, n:] = np.nan                                     # the whole mel and z of the row of 0 frames
        z[b, n * hop:] = np.nan
    assert 0 in c.frames and np.isnan(mel[:, -1]).sum() > 0 and np.abs(wav).max() > 0
    got, got_len = v(mel, c.frames_array, z=z, sigma=c.sigma)
    assert np.array_equal(got_len, lengths) and np.array_equal(got.view(np.int32), wav.view(np.int32))
    for b, n in enumerate(lengths):
        assert not got[b, n:].any(), b


def test_a_row_of_nan_leaves_its_neighbours_bitwise_alone():
    """One row's mel is NaN inside its own length: every other row is bitwise the row run alone; the bad row may hold anything up
    to its length and holds zeros beyond it."""
    c = M.CASES["tiny"]
    v = _vocoder("tiny")
    hop = c.cfg.hop
    mel, frames = c.mel.copy(), c.frames_array.copy()
    frames[0] = c.frames[0] - 1                                 # the bad row is the longest: leave room beyond it
    mel[0, frames[0] // 2, 1] = np.nan
    wav, lengths = v(mel, frames, z=c.z, sigma=c.sigma)
    assert np.array_equal(lengths, frames * hop) and not wav[0, lengths[0]:].any()
    for b in range(1, len(frames)):
        n = int(frames[b])
        assert not wav[b, lengths[b]:].any()
        if n >= 1:
            alone, alone_len = v(c.mel[b:b + 1, :n], z=c.z[b:b + 1, :n * hop], sigma=c.sigma)
            assert alone_len[0] == lengths[b] and np.array_equal(alone[0].view(np.int32), wav[b, :lengths[b]].view(np.int32)), b


# ---------------------------------------------------------------------------------------------------- 3. the noise
def test_the_noise_is_the_host_box_muller():
    """z[b, l * G + g] = Box-Muller of the x and y words of Philox counter (l, g, 0, 0x8000) under seeds[b]: oracle/rng_np.py's words,
    float64 Box-Muller on the same float32 uniforms.  The device's __logf / __cosf are not bitwise that; the bound is 4 x the error
    measured on an MI355X (NOISE_ERR_MEASURED above: 8.70e-7 / 8.30e-7 on tiny's two seeds, 8.13e-7 / 5.05e-7 on early_g16's, with
    max |z| up to 3.14; the bound is 3.48e-6)."""
    for name in ("tiny", "early_g16"):
        c = M.CASES[name]
        v = _vocoder(name)
        G, T = c.cfg.n_group, c.T
        L = T * c.cfg.hop // G
        seeds = [SEED, 3]
        z = v.noise(seeds, T)
        l, g = np.arange(L)[:, None], np.arange(G)[None, :]
        for b, seed in enumerate(seeds):
            x, y, _, _ = rng_np.philox4x32_10(seed, l, g, 0, STREAM_WAVEGLOW)
            want = rng_np.normal(x, y).reshape(-1)
            err = float(np.abs(z[b].astype(np.float64) - want).max())
            print("waveglow noise", name, "seed", hex(seed), "max abs error against float64 Box-Muller", err, "max |z|", float(np.abs(z[b]).max()))
            assert err <= NOISE_TOL and np.abs(z[b]).max() <= 5.8


# ---------------------------------------------------------------------------------------------------- 4. sigma
def test_sigma_zero_is_deterministic_and_sigma_scales_the_noise():
    c = M.CASES["tiny"]
    v = _vocoder("tiny")
    want0, want_len, _ = M.reference("tiny", "float64", 0.0)
    bar0 = K * M.e32("tiny", 0.0)
    a, lens = v(c.mel, c.frames_array, seeds=[1, 2, 3, 4], sigma=0.0)
    b, _ = v(c.mel, c.frames_array, z=c.z, sigma=0.0)
    assert np.array_equal(a, b) and np.array_equal(lens, want_len)                             # no noise reaches the output
    assert _worst(a, want0, want_len, "sigma 0") <= bar0 and np.abs(a).max() > 0.1
    half, _ = v(c.mel, c.frames_array, z=c.z * np.float32(0.5), sigma=1.0)                     # (halving a float32 is exact)
    low, _ = v(c.mel, c.frames_array, z=c.z, sigma=0.5)
    want, _, _ = M.reference("tiny", "float64", 0.5)
    bar = K * M.e32("tiny", 0.5)
    assert _worst(half, want, want_len, "z / 2") <= bar and _worst(low, want, want_len, "sigma 0.5") <= bar
    assert np.abs(half.astype(np.float64) - low).max() <= 2 * bar


# ---------------------------------------------------------------------------------------------------- 5. refusals through the C ABI
def test_refusals_come_through_the_c_abi():
    import torch
    c = M.CASES["tiny"]
    hop = c.cfg.hop
    raw = _Vocoder(c.cfg, c.weights, 2, 9, finalize=False)
    try:
        x = torch.zeros((3, 10, c.cfg.mel_dim), dtype=torch.float32, device="cuda")
        z = torch.zeros((3, 10 * hop), dtype=torch.float32, device="cuda")
        sd = _seeds([1, 2, 3])
        wav = torch.zeros((3, 10 * hop), dtype=torch.float32, device="cuda")
        err = lambda: raw.ctx.lib.gsttaco_last_error(raw.ctx.handle).decode()
        assert raw.raw(x, None, 1, 9, 0.6, None, z, wav, None, 9 * hop) == -4 and "finalize" in err()     # a run before finalize
        with pytest.raises(capi.GstTacoError) as e:                                                   # a wrong shape
            raw.ctx.waveglow_load_weight("waveglow/flow0/W", np.zeros((8, 7), np.float32))
        assert e.value.code == -4
        singular = np.array(c.weights["waveglow/flow1/W"])
        singular[3] = singular[2]
        raw.ctx.waveglow_load_weight("waveglow/flow1/W", singular)
        with pytest.raises(capi.GstTacoError) as e:                                                   # a W that has no inverse
            raw.ctx.waveglow_finalize()
        assert e.value.code == -4 and "singular" in str(e.value)
        raw.ctx.waveglow_load_weight("waveglow/flow1/W", c.weights["waveglow/flow1/W"])
        raw.ctx.waveglow_finalize()
        with pytest.raises(capi.GstTacoError) as e:                                                   # a load after finalize
            raw.ctx.waveglow_load_weight("waveglow/up/bias", np.zeros((c.cfg.mel_dim,), np.float32))
        assert e.value.code == -4
        assert raw.raw(x, None, 3, 9, 0.6, None, z, wav, None, 9 * hop) == -5 and "capacity" in err()    # B over the capacity
        assert raw.raw(x, None, 2, 10, 0.6, None, z, wav, None, 10 * hop) == -5                           # T over the capacity
        assert raw.raw(x, None, 2, 9, 0.6, None, z, wav, None, 9 * hop - 1) == -1 and "ld_wav" in err()  # a short ld_wav
        assert raw.raw(None, None, 2, 9, 0.6, None, z, wav, None, 9 * hop) == -1
        assert raw.raw(x, None, 2, 9, 0.6, None, z, None, None, 9 * hop) == -1
        assert raw.raw(x, None, 0, 9, 0.6, None, z, wav, None, 9 * hop) == -1
        assert raw.raw(x, None, 2, 0, 0.6, None, z, wav, None, 9 * hop) == -1
        assert raw.raw(x, None, 2, 9, 0.6, sd, z, wav, None, 9 * hop) == -1 and "one of" in err()        # both seeds and z
        assert raw.raw(x, None, 2, 9, 0.6, None, None, wav, None, 9 * hop) == -1 and "one of" in err()   # neither
        assert raw.raw(x, None, 2, 9, -0.1, None, z, wav, None, 9 * hop) == -1 and "sigma" in err()
        assert raw.raw(x, None, 2, 9, float("nan"), None, z, wav, None, 9 * hop) == -1
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        noise = raw.ctx.lib.gsttaco_waveglow_noise
        assert noise(raw.ctx.handle, None, 2, 9, ctypes.c_void_p(z.data_ptr()), s) == -1
        assert noise(raw.ctx.handle, ctypes.c_void_p(sd.data_ptr()), 0, 9, ctypes.c_void_p(z.data_ptr()), s) == -1
        torch.cuda.synchronize()
        assert not wav.any().item() and not z.any().item()                                           # nothing was written
        assert raw.raw(x, None, 2, 9, 0.6, sd, None, wav, None, 9 * hop) == 0                         # and the context still runs
        torch.cuda.synchronize()
        assert wav[:2, :9 * hop].abs().max().item() > 0
    finally:
        raw.close()
    ctx = capi.Context(synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4)
    try:                                                                                              # configure's refusals, as on the CPU
        for kwargs, field in ((dict(win=1000), "win"), (dict(hop=252, win=1008), "hop"), (dict(n_group=7, hop=252, win=1008), "n_group"),
                              (dict(n_early_size=1), "n_early_size"), (dict(n_early_size=4), "n_early_size"), (dict(n_layers=11), "n_layers"),
                              (dict(n_flows=33, n_early_every=64), "n_flows"), (dict(n_group=18, hop=252, win=1008), "n_group"),
                              (dict(n_channels=0), "n_channels"), (dict(n_channels=1024), "LDS")):
            with pytest.raises(capi.GstTacoError) as e:
                ctx.waveglow_configure(waveglow.WaveGlowConfig(**kwargs), 2, 16)
            assert e.value.code == -1 and field in str(e.value), (kwargs, str(e.value))
        ctx.waveglow_configure(waveglow.WaveGlowConfig(), 2, 16)
        with pytest.raises(capi.GstTacoError) as e:
            ctx.waveglow_configure(waveglow.WaveGlowConfig(), 2, 16)
        assert e.value.code == -1 and "already" in str(e.value)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------- 6. end to end
def _tiny_model(tmp_path, tag):
    from gst_tacotron_amd import weights
    from gst_tacotron_amd.model import GST_Tacotron
    hp = synthetic.tiny_hp(max_step=24)
    hp["Inference_Path"] = str(tmp_path / tag)
    hp["Vocoder_Taco1"]["Griffin-Lim_Iter"] = 3
    m = GST_Tacotron(hyper_parameters=hp, max_batch=2, max_tokens=16, max_ref_frames=200, max_wav_seconds=1.0)
    m.Restore(weights=weights.synthetic_weights(hp, seed=2))
    return m, hp


def _wav_bytes(hp, label, i):
    return open(os.path.join(hp["Inference_Path"], "Wav", "%s.IDX_%d.WAV" % (label, i)), "rb").read()


def test_inference_exports_through_the_flow_vocoder_and_the_other_paths_are_untouched(tmp_path):
    import torch
    import wave
    rng = np.random.default_rng(0)
    ref_mel = np.clip(rng.normal(0, 1.5, (40, 16)), -4, 4).astype(np.float32)
    sents, seeds = ["Hi there.", "Yes."], [11, 12]
    mg_cfg = melgan.MelGANConfig(mel_dim=16, base=4, ratios=[4, 2, 2], n_res=2)       # 4 * 2 * 2 = the tiny Frame_Shift
    m, hp = _tiny_model(tmp_path, "plain")
    try:
        m.Load_Neural_Vocoder(melgan.synthetic_weights(mg_cfg, seed=8), max_frames=24)
        m.Inference(sents, [ref_mel], label="G", export=True, seeds=seeds)
        m.Inference(sents, [ref_mel], label="M", export=True, seeds=seeds, vocoder="melgan")
        plain = {lab: [_wav_bytes(hp, lab, i) for i in range(2)] for lab in ("G", "M")}
        with pytest.raises(capi.GstTacoError) as e:                                     # before Load_WaveGlow
            m.Inference(sents, [ref_mel], label="W", export=True, seeds=seeds, vocoder="waveglow")
        assert e.value.code == -4 and "Load_WaveGlow" in str(e.value)
    finally:
        m.ctx.close()
    hop = hp["Sound"]["Frame_Shift"]
    cfg = waveglow.WaveGlowConfig(mel_dim=16, hop=hop, win=2 * hop, n_group=4, n_flows=3, n_early_every=2, n_layers=2, n_channels=16)
    m, hp = _tiny_model(tmp_path, "voc")
    try:
        with pytest.raises(ValueError, match="Frame_Shift"):
            m.Load_WaveGlow(waveglow.synthetic_weights(cfg, seed=8), config=waveglow.WaveGlowConfig(**dict(cfg.__dict__, hop=hop // 2, win=hop)))
        m.Load_Neural_Vocoder(melgan.synthetic_weights(mg_cfg, seed=8), max_frames=24)
        m.Load_WaveGlow(waveglow.synthetic_weights(cfg, seed=8), max_frames=24)         # the sizes come from the arrays' shapes
        assert m._waveglow == cfg
        m.Inference(sents, [ref_mel], label="G", export=True, seeds=seeds)              # the default: Griffin-Lim
        m.Inference(sents, [ref_mel], label="M", export=True, seeds=seeds, vocoder="melgan")
        assert {lab: [_wav_bytes(hp, lab, i) for i in range(2)] for lab in ("G", "M")} == plain
        out = m.Inference(sents, [ref_mel], label="W", export=True, seeds=seeds, vocoder="waveglow")
        report, _ = m.Utterance_Report(out[1], out[3])
        frames = report[:, 1].contiguous()
        wav, lens = m.WaveGlow(out[0], frames, seeds=seeds)
        host = m.WaveGlow(out[0].cpu().numpy(), frames.cpu().numpy(), seeds=np.asarray(seeds))          # host arrays: the same bits
        z = torch.zeros((2, out[0].shape[1] * hop), dtype=torch.float32, device=wav.device)
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        m.ctx.check(m.ctx.lib.gsttaco_waveglow_noise(m.ctx.handle, ctypes.c_void_p(_seeds(seeds).data_ptr()), 2, out[0].shape[1],
                                                     ctypes.c_void_p(z.data_ptr()), s))
        by_z = m.WaveGlow(out[0], frames, z=z)
        unseeded, _ = m.WaveGlow(out[0], frames)
        zero, _ = m.WaveGlow(out[0], frames, seeds=[0, 0])
        torch.cuda.synchronize()
        assert torch.equal(host[0], wav) and torch.equal(host[1], lens) and torch.equal(by_z[0], wav)
        assert torch.equal(unseeded, zero) and not torch.equal(zero, wav)                # seeds=None: seed 0 for every row
        with pytest.raises(ValueError):
            m.WaveGlow(out[0], frames, seeds=seeds, z=z)
        wav, lens, frames = wav.cpu().numpy(), lens.cpu().numpy(), frames.cpu().numpy()
        assert np.array_equal(lens, frames * hop) and lens.min() > 0
        for i in range(2):
            with wave.open(os.path.join(hp["Inference_Path"], "Wav", "W.IDX_%d.WAV" % i), "rb") as f:
                assert f.getframerate() == 16000 and f.getsampwidth() == 2
                pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
            want = np.clip(wav[i, :lens[i]].astype(np.float64) * 32768.0, -32768, 32767).astype("<i2")
            assert len(pcm) == frames[i] * hop and np.array_equal(pcm, want) and _wav_bytes(hp, "W", i) not in plain["G"] + plain["M"]
    finally:
        m.ctx.close()
