"""GPU tests of the neural vocoder (csrc/melgan.hip through gsttaco_melgan): every case of tests/melgan_cases.py against the float64
restatement, row by row over the row's length, to K times the case's own float32-restatement error; lengths, the zeros beyond a row
and the short rows exactly; the bitwise properties the header promises (a row alone, a larger capacity, host arrays, a repeated
call, a captured graph); every refusal straight through the C ABI; and Inference(export=True, vocoder="melgan") end to end.

The measured ratios of device error to e32 stand at test_every_case_equals_the_float64_restatement_row_by_row and in DESIGN 3.5."""
import ctypes
import os

import numpy as np
import pytest

import melgan_cases as M
from vocoder_harness import Vocoder
from gst_tacotron_amd import capi, melgan, synthetic

pytestmark = pytest.mark.gpu

# The bar is K * e32(case).  The device and the float32 restatement are fp32 chains of one depth that differ in summation order only;
# K is the smallest power of two at least twice the largest measured ratio (1.61, the docstring of test_every_case...), never above 16.
K = 4

_VOCODERS = {}


def _Vocoder(cfg, weights, max_batch, max_frames, finalize=True):
    """A context that holds nothing but a finalized vocoder."""
    return Vocoder("melgan", cfg, weights, max_batch, max_frames, finalize)


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
    """Largest device error over the case's rows / e32(case), measured on an MI355X: tiny 0.63 (3.7e-7 / 6.0e-7), odd_channels 1.16
    (2.5e-7 / 2.1e-7), min_rows 1.45 (8.4e-7 / 5.8e-7), dilation_edge 1.09 (1.8e-7 / 1.6e-7), tiles 1.61 (5.2e-6 / 3.3e-6),
    full_size 1.45 (8.7e-6 / 6.0e-6), hot 1.00 (4.8e-7 / 4.8e-7).  Twice the largest is 3.2: K = 4."""
    c = M.CASES[name]
    want, want_len = M.reference(name)
    e32 = M.e32(name)
    v = _vocoder(name)
    if name == "tiles":         # the case's rows come from the tiles the library really uses
        min_frames, hop, stages = v.ctx.melgan_plan()
        tiles = [(s["kind"], s["channels"], s["tile"], s["form"], s["rate"]) for s in stages]
        assert tiles == M.plan_tiles(c.cfg) and tuple(M.tile_edge_frames(tiles, min_frames)) == c.frames
    wav, lengths = v(c.mel, c.frames_array)
    assert np.array_equal(lengths, want_len)
    assert np.isfinite(wav).all() and np.abs(wav).max() <= 1.0
    worst = 0.0
    for b, n in enumerate(want_len):
        assert not wav[b, n:].any(), (name, b)                  # zeros beyond the row, exactly; a short row is all zeros
        if n:
            worst = max(worst, float(np.abs(wav[b, :n].astype(np.float64) - want[b, :n]).max()))
    print("melgan case", name, "device error", worst, "e32", e32, "ratio", worst / e32)
    assert worst <= K * e32
    assert (want_len == 0).sum() == sum(n < c.cfg.min_frames for n in c.frames)


# ---------------------------------------------------------------------------------------------------- 2. bitwise properties
@pytest.mark.parametrize("name", ["tiny", "tiles", "full_size"])
def test_a_call_repeats_and_a_row_in_its_batch_is_the_row_alone(name):
    c = M.CASES[name]
    v = _vocoder(name)
    wav, lengths = v(c.mel, c.frames_array)
    again, _ = v(c.mel, c.frames_array)
    assert np.array_equal(wav, again)
    rows = [b for b, n in enumerate(c.frames) if n >= c.cfg.min_frames]
    for b in rows[:2] + rows[-3:]:
        n = c.frames[b]
        alone, alone_len = v(c.mel[b:b + 1, :n])                # B = 1, T = its frames, no lengths
        assert alone_len[0] == lengths[b] == n * c.cfg.hop and np.array_equal(alone[0], wav[b, :lengths[b]]), (name, b)
    wide, _ = v(c.mel, c.frames_array, ld=c.T * c.cfg.hop + 37)  # a wider wav: the same samples, zeros in the extra columns
    assert np.array_equal(wide[:, :wav.shape[1]], wav) and not wide[:, wav.shape[1]:].any()


def test_a_large_call_leaves_nothing_behind_for_a_small_one():
    """Capacity 4 x 160 frames: a full-capacity call, then a small one, against the small one on a fresh context of exactly its
    size -- stale workspace behind a row's end must not leak in."""
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


def _nan_beyond(mel, frames, min_frames):
    """the mel with NaN beyond each row's frames, and in the whole mel of a row too short to run"""
    out = np.array(mel, dtype=np.float32)
    for b, n in enumerate(frames):
        out[b, (n if n >= min_frames else 0):] = np.nan
    return out


def test_nan_beyond_a_row_reaches_no_sample():
    """What lies beyond a row's frames -- in Inference(..., vocoder=) the decoder's free run past the stop token -- may be NaN: a
    bound taken as a product passes a finite filler and fails this.  The wav and the lengths are bitwise those of the plain call."""
    c = M.CASES["tiny"]
    v = _vocoder("tiny")
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    for frames in (c.frames_array, np.asarray([0, c.cfg.min_frames - 1, 6], dtype=np.int32)):
        wav, lengths = v(c.mel, frames)
        mel = _nan_beyond(c.mel, frames, c.cfg.min_frames)
        assert np.isnan(mel).any() and np.abs(wav).max() > 0
        got, got_len = v(mel, frames)
        assert np.array_equal(got_len, lengths) and np.array_equal(bits(got), bits(wav))
        for b, n in enumerate(lengths):
            assert not got[b, n:].any(), b


def test_a_row_of_nan_leaves_its_neighbours_bitwise_alone():
    """One row's mel is NaN inside its own length: every other row is bitwise the row run alone; the bad row may hold anything up
    to its length and holds zeros beyond it."""
    c = M.CASES["tiny"]
    v = _vocoder("tiny")
    mel, frames = c.mel.copy(), c.frames_array.copy()
    frames[0] = c.frames[0] - 1                                 # the bad row is the longest: leave room beyond it
    mel[0, frames[0] // 2, 1] = np.nan
    wav, lengths = v(mel, frames)
    assert np.array_equal(lengths, frames * c.cfg.hop) and not wav[0, lengths[0]:].any()
    for b in range(1, len(frames)):
        n = int(frames[b])
        alone, alone_len = v(c.mel[b:b + 1, :n])
        assert alone_len[0] == lengths[b] and np.array_equal(alone[0].view(np.int32), wav[b, :lengths[b]].view(np.int32)), b
        assert not wav[b, lengths[b]:].any()


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
            raw.ctx.melgan_load_weight("melgan/out/kernel", np.zeros((7 * c.cfg.base, 2), np.float32))
        assert e.value.code == -4
        raw.ctx.melgan_finalize()
        with pytest.raises(capi.GstTacoError) as e:                                                   # a load after finalize
            raw.ctx.melgan_load_weight("melgan/out/bias", np.zeros((1,), np.float32))
        assert e.value.code == -4
        assert raw.raw(x, None, 3, 9, wav, None, 9 * c.cfg.hop) == -5 and "capacity" in err()        # B over the capacity
        assert raw.raw(x, None, 2, 10, wav, None, 10 * c.cfg.hop) == -5                               # T over the capacity
        assert raw.raw(x, None, 2, 9, wav, None, 9 * c.cfg.hop - 1) == -1 and "ld_wav" in err()      # a short ld_wav
        assert raw.raw(None, None, 2, 9, wav, None, 9 * c.cfg.hop) == -1
        assert raw.raw(x, None, 0, 9, wav, None, 9 * c.cfg.hop) == -1
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
    cfg = melgan.MelGANConfig(mel_dim=16, base=4, ratios=[4, 2, 2], n_res=2)        # 4 * 2 * 2 = the tiny Frame_Shift
    m, hp = _tiny_model(tmp_path, "voc")
    try:
        with pytest.raises(ValueError, match="Frame_Shift"):
            m.Load_Neural_Vocoder(melgan.synthetic_weights(melgan.MelGANConfig(mel_dim=16, base=4, ratios=[2, 2], n_res=2), seed=8))
        m.Load_Neural_Vocoder(melgan.synthetic_weights(cfg, seed=8), max_frames=24)
        m.Inference(sents, [ref_mel], label="G", export=True, seeds=seeds)                              # the default: Griffin-Lim
        assert [_wav_bytes(hp, "G", i) for i in range(2)] == plain
        out = m.Inference(sents, [ref_mel], label="M", export=True, seeds=seeds, vocoder="melgan")
        report, _ = m.Utterance_Report(out[1], out[3])
        wav, lens = m.Neural_Vocoder(out[0], report[:, 1].contiguous())
        host = m.Neural_Vocoder(out[0].cpu().numpy(), report[:, 1].cpu().numpy())                       # host arrays: the same bits
        torch.cuda.synchronize()
        assert torch.equal(host[0], wav) and torch.equal(host[1], lens)
        wav, lens, frames = wav.cpu().numpy(), lens.cpu().numpy(), report[:, 1].cpu().numpy()
        assert np.array_equal(lens, [f * cfg.hop if f >= cfg.min_frames else 0 for f in frames]) and lens.max() > 0
        for i in range(2):
            with wave.open(os.path.join(hp["Inference_Path"], "Wav", "M.IDX_%d.WAV" % i), "rb") as f:
                assert f.getframerate() == 16000 and f.getsampwidth() == 2
                pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
            want = np.clip(wav[i, :lens[i]].astype(np.float64) * 32768.0, -32768, 32767).astype("<i2")
            assert np.array_equal(pcm, want) and _wav_bytes(hp, "M", i) != plain[i]
    finally:
        m.ctx.close()
