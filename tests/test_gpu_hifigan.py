"""GPU tests of the HiFi-GAN vocoder (csrc/hifigan.hip through gsttaco_hifigan): every case of tests/hifigan_cases.py against the
float64 restatement, row by row over the row's length, to K times the case's own float32-restatement error; lengths and the zeros
beyond a row exactly; the bitwise properties the header promises (a row alone, a larger capacity, host arrays, a repeated call, a
wider wav, a captured graph); every refusal straight through the C ABI; and Inference(export=True, vocoder="hifigan") end to end.

The measured ratios of device error to e32 stand at test_every_case_equals_the_float64_restatement_row_by_row and in DESIGN 3.5."""
import ctypes
import os

import numpy as np
import pytest

import hifigan_cases as M
from vocoder_harness import Vocoder
from gst_tacotron_amd import capi, hifigan, melgan, synthetic

pytestmark = pytest.mark.gpu

# The bar is K * e32(case).  The device and the float32 restatement are fp32 chains of one depth that differ in summation order only.
# K was set before any run, at the larger of the two bars the project holds for the same kind of chain on the same MFMA path (MelGAN 4,
# WaveGlow 8): V1's depth, 24 convolutions in sequence plus the fusion sums, lies between theirs.
K = 8

_VOCODERS = {}


def _Vocoder(cfg, weights, max_batch, max_frames, finalize=True):
    """A context that holds nothing but a finalized HiFi-GAN."""
    return Vocoder("hifigan", cfg, weights, max_batch, max_frames, finalize)


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


# ---------------------------------------------------------------------------------------------------- 1. every case against float64
@pytest.mark.parametrize("name", M.NAMES)
def test_every_case_equals_the_float64_restatement_row_by_row(name):
    """Largest device error over the case's rows / e32(case), measured on an MI355X: tiny 1.09 (1.4e-7 / 1.3e-7), odd_channels 0.83
    (2.5e-7 / 3.0e-7), one_kernel 1.58 (4.3e-7 / 2.7e-7), one_kernel_v3 1.18 (2.3e-7 / 2.0e-7), halo 0.88 (8.1e-7 / 9.3e-7), tiles
    2.20 (6.6e-6 / 3.0e-6), v1 1.88 (9.1e-6 / 4.9e-6), v3 1.49 (4.0e-6 / 2.7e-6), hot 1.60 (3.8e-6 / 2.4e-6).  None is above 4."""
    c = M.CASES[name]
    want, want_len = M.reference(name)
    e32 = M.e32(name)
    v = _vocoder(name)
    if name == "tiles":         # the case's rows come from the tiles the library really uses
        min_frames, hop, stages = v.ctx.hifigan_plan()
        tiles = [(s["kind"], s["channels"], s["taps"], s["dilation"], s["tile"], s["form"], s["rate"]) for s in stages]
        assert min_frames == 1 and tiles == M.plan_tiles(c.cfg) and tuple(M.tile_edge_frames(tiles)) == c.frames
    wav, lengths = v(c.mel, c.frames_array)
    assert np.array_equal(lengths, want_len)
    assert np.isfinite(wav).all() and np.abs(wav).max() <= 1.0
    worst = 0.0
    for b, n in enumerate(want_len):
        assert not wav[b, n:].any(), (name, b)                  # zeros beyond the row, exactly; an empty row is all zeros
        if n:
            worst = max(worst, float(np.abs(wav[b, :n].astype(np.float64) - want[b, :n]).max()))
    print("hifigan case", name, "device error", worst, "e32", e32, "ratio", worst / e32)
    assert worst <= K * e32
    assert (want_len == 0).sum() == sum(n < 1 for n in c.frames)


# ---------------------------------------------------------------------------------------------------- 2. bitwise properties
@pytest.mark.parametrize("name", ["tiny", "odd_channels", "halo", "tiles", "v1", "v3"])
def test_a_call_repeats_and_a_row_in_its_batch_is_the_row_alone(name):
    c = M.CASES[name]
    v = _vocoder(name)
    wav, lengths = v(c.mel, c.frames_array)
    again, _ = v(c.mel, c.frames_array)
    assert np.array_equal(wav, again)
    rows = [b for b, n in enumerate(c.frames) if n >= 1]
    for b in sorted(set(rows[:3] + rows[-3:])):
        n = c.frames[b]
        alone, alone_len = v(c.mel[b:b + 1, :n])                # B = 1, T = its frames, no lengths
        assert alone_len[0] == lengths[b] == n * c.cfg.hop and np.array_equal(alone[0], wav[b, :lengths[b]]), (name, b)
    wide, _ = v(c.mel, c.frames_array, ld=c.T * c.cfg.hop + 37)  # a wider wav: the same samples, zeros in the extra columns
    assert np.array_equal(wide[:, :wav.shape[1]], wav) and not wide[:, wav.shape[1]:].any()
    over, over_len = v(c.mel, c.frames_array + 1000 * (c.frames_array == c.T))      # frames above T count as T
    assert np.array_equal(over, wav) and np.array_equal(over_len, lengths)


def test_a_large_call_leaves_nothing_behind_for_a_small_one():
    """Capacity 4 x 160 frames: a full-capacity call, then a small one, against the small one on a fresh context of exactly its
    size -- stale workspace behind a row's end, in any of the four buffers, must not leak in."""
    c = M.CASES["tiles"]
    rng = np.random.default_rng(9)
    big = _Vocoder(c.cfg, c.weights, 4, 160)
    try:
        full, full_len = big(np.clip(rng.normal(0, 1.5, (4, 160, c.cfg.mel_dim)), -4, 4))
        assert (full_len == 160 * c.cfg.hop).all() and np.abs(full).max() > 0.1
        small_mel = np.clip(rng.normal(0, 1.5, (2, 9, c.cfg.mel_dim)), -4, 4).astype(np.float32)
        got = big(small_mel, [5, 9])
    finally:
        big.close()
    fresh = _Vocoder(c.cfg, c.weights, 2, 9)
    try:
        want = fresh(small_mel, [5, 9])
    finally:
        fresh.close()
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]) and np.abs(want[0]).max() > 0.1


def test_the_call_is_captured_in_a_graph_and_replays_bitwise():
    """No allocation and no synchronisation inside the call: it is captured on a side stream and replayed twice."""
    import torch
    c = M.CASES["tiny"]
    v = _vocoder("tiny")
    eager, eager_len = v(c.mel, c.frames_array)
    x = torch.as_tensor(c.mel).cuda()
    fr = torch.as_tensor(c.frames_array).cuda()
    B, T = x.shape[:2]
    ld = T * c.cfg.hop
    wav = torch.full((B, ld), float("nan"), dtype=torch.float32, device="cuda")
    lens = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = v.raw(x, fr, B, T, wav, lens, ld)
    assert rc == 0
    for _ in range(2):
        wav.fill_(float("nan"))
        lens.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(wav.cpu().numpy(), eager) and np.array_equal(lens.cpu().numpy(), eager_len)


# ---------------------------------------------------------------------------------------------------- 3. refusals through the C ABI
def test_refusals_come_through_the_c_abi():
    import torch
    c = M.CASES["tiny"]
    raw = _Vocoder(c.cfg, c.weights, 2, 9, finalize=False)
    try:
        x = torch.zeros((3, 10, c.cfg.mel_dim), dtype=torch.float32, device="cuda")
        wav = torch.zeros((3, 10 * c.cfg.hop), dtype=torch.float32, device="cuda")
        err = lambda: raw.ctx.lib.gsttaco_last_error(raw.ctx.handle).decode()
        assert raw.raw(x, None, 1, 9, wav, None, 9 * c.cfg.hop) == -4 and "finalize" in err()       # a run before finalize
        with pytest.raises(capi.GstTacoError) as e:                                                   # a wrong shape
            raw.ctx.hifigan_load_weight("hifigan/out/kernel", np.zeros((7 * c.cfg.channels()[-1], 2), np.float32))
        assert e.value.code == -4
        raw.ctx.hifigan_finalize()
        with pytest.raises(capi.GstTacoError) as e:                                                   # a load after finalize
            raw.ctx.hifigan_load_weight("hifigan/out/bias", np.zeros((1,), np.float32))
        assert e.value.code == -4
        assert raw.raw(x, None, 3, 9, wav, None, 9 * c.cfg.hop) == -5 and "capacity" in err()        # B over the capacity
        assert raw.raw(x, None, 2, 10, wav, None, 10 * c.cfg.hop) == -5                               # T over the capacity
        assert raw.raw(x, None, 2, 9, wav, None, 9 * c.cfg.hop - 1) == -1 and "ld_wav" in err()      # a short ld_wav
        assert raw.raw(None, None, 2, 9, wav, None, 9 * c.cfg.hop) == -1
        assert raw.raw(x, None, 2, 9, None, None, 9 * c.cfg.hop) == -1
        assert raw.raw(x, None, 0, 9, wav, None, 9 * c.cfg.hop) == -1
        assert raw.raw(x, None, 2, 0, wav, None, 9 * c.cfg.hop) == -1
        torch.cuda.synchronize()
        assert not wav.any().item()                                                                   # nothing was written
        assert raw.raw(x, None, 2, 9, wav, None, 9 * c.cfg.hop) == 0                                  # and the context still runs
        torch.cuda.synchronize()
        assert wav[:2, :9 * c.cfg.hop].abs().max().item() > 0
    finally:
        raw.close()


# ---------------------------------------------------------------------------------------------------- 4. end to end
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


def test_inference_exports_through_the_vocoder_and_the_default_path_is_untouched(tmp_path):
    import torch
    import wave
    rng = np.random.default_rng(0)
    ref_mel = np.clip(rng.normal(0, 1.5, (40, 16)), -4, 4).astype(np.float32)
    sents, seeds = ["Hi there.", "Yes."], [11, 12]
    m, hp = _tiny_model(tmp_path, "plain")
    try:
        m.Inference(sents, [ref_mel], label="G", export=True, seeds=seeds)
        plain = [_wav_bytes(hp, "G", i) for i in range(2)]
    finally:
        m.ctx.close()
    # 4 * 2 * 2 = the tiny Frame_Shift; the dilations are no shipped shape, so the configuration is given
    cfg = hifigan.HiFiGANConfig(mel_dim=16, initial=16, rates=[4, 2, 2], resblock=1, kernels=[3, 5], dilations=[[1, 2], [3]])
    m, hp = _tiny_model(tmp_path, "voc")
    try:
        short = hifigan.HiFiGANConfig(mel_dim=16, initial=16, rates=[2, 2], resblock=1, kernels=[3], dilations=[[1]])
        with pytest.raises(ValueError, match="Frame_Shift"):
            m.Load_HiFiGAN(hifigan.synthetic_weights(short, seed=8), config=short)
        with pytest.raises(ValueError, match="dilations"):
            m.Load_HiFiGAN(hifigan.synthetic_weights(cfg, seed=8))
        m.Load_HiFiGAN(hifigan.synthetic_weights(cfg, seed=8), config=cfg, max_frames=24)
        m.Inference(sents, [ref_mel], label="G", export=True, seeds=seeds)                              # the default: Griffin-Lim
        assert [_wav_bytes(hp, "G", i) for i in range(2)] == plain
        out = m.Inference(sents, [ref_mel], label="H", export=True, seeds=seeds, vocoder="hifigan")
        report, _ = m.Utterance_Report(out[1], out[3])
        wav, lens = m.HiFiGAN(out[0], report[:, 1].contiguous())
        host = m.HiFiGAN(out[0].cpu().numpy(), report[:, 1].cpu().numpy())                              # host arrays: the same bits
        torch.cuda.synchronize()
        assert torch.equal(host[0], wav) and torch.equal(host[1], lens)
        wav, lens, frames = wav.cpu().numpy(), lens.cpu().numpy(), report[:, 1].cpu().numpy()
        assert np.array_equal(lens, [f * cfg.hop for f in frames]) and lens.max() > 0
        for i in range(2):
            with wave.open(os.path.join(hp["Inference_Path"], "Wav", "H.IDX_%d.WAV" % i), "rb") as f:
                assert f.getframerate() == 16000 and f.getsampwidth() == 2
                pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
            want = np.clip(wav[i, :lens[i]].astype(np.float64) * 32768.0, -32768, 32767).astype("<i2")
            assert np.array_equal(pcm, want) and _wav_bytes(hp, "H", i) != plain[i]
        # MelGAN still loads and works in the same context, and leaves the HiFi-GAN's samples as they were
        mcfg = melgan.MelGANConfig(mel_dim=16, base=4, ratios=[4, 2, 2], n_res=2)
        m.Load_Neural_Vocoder(melgan.synthetic_weights(mcfg, seed=8), max_frames=24)
        m.Inference(sents, [ref_mel], label="M", export=True, seeds=seeds, vocoder="melgan")
        assert all(_wav_bytes(hp, "M", i) not in (plain[i], _wav_bytes(hp, "H", i)) for i in range(2))
        again, _ = m.HiFiGAN(out[0], report[:, 1].contiguous())
        torch.cuda.synchronize()
        assert np.array_equal(again.cpu().numpy(), wav)
        with pytest.raises(ValueError):
            m.Inference(sents, [ref_mel], export=True, vocoder="wavenet")
    finally:
        m.ctx.close()
