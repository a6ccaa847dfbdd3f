"""GPU test of the seam between the phase entry points and the whole call: encode -> Inference_GST_Step -> decode -> postnet stages its
decode inputs (injected masks with the padded decoder's re-layout, injected noise, the teacher frames) and keys its graph segments on
its own, Inference_Step does the same inside one call -- with the same inputs the two must give the same bits, at the first use of
every graph and at its replay, and gsttaco_debug_randomness must hand the injected masks back in the caller's layout after either.
In front of each path the OTHER path runs with other masks, noise and teacher frames, so a staging step that silently did nothing
would leave those in the workspace and show in the outputs and in the read-back."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, TV, TREF, STEPS, R = 3, 9, 5, 6, 2
TQ = R * STEPS + 1

# synthetic.tiny_hp's decoder (prenet 32 / 32, attention 16, LSTM 64 / 64) is below the reference's sizes, so finalize zero-pads it
# (pad_decoder) unless GSTTACO_PAD_DECODER=0 keeps its own sizes; the third case pads from other sizes, none equal to the tiny model's
CASES = {"tiny-padded": (None, "1"), "tiny-own-sizes": (None, "0"), "other-sizes-padded": (([48, 48], 32, [96, 80]), "1")}


def _case(name):
    from gst_tacotron_amd import synthetic, weights
    sizes, pad = CASES[name]
    hp = synthetic.tiny_hp("SMA", r=R, gst=True)
    if sizes:
        dec = hp["Tacotron2"]["Decoder"]
        dec["Prenet"]["Size"], dec["Attention"]["Size"], dec["RNN"]["Size"] = list(sizes[0]), sizes[1], list(sizes[2])
    prenet = hp["Tacotron2"]["Decoder"]["Prenet"]["Size"]
    rng = np.random.default_rng(31)
    tokens, tl = synthetic.make_tokens(rng, B, TV)
    mels, ml = synthetic.make_ref_mels(rng, B, TREF, mel=16, lengths=np.array([5, 3, 4]))
    masks, noise = synthetic.make_randomness(rng, STEPS, B, TV, prenet)      # (the caller's prenet sizes)
    teacher = np.clip(rng.normal(0.0, 1.5, (B, TQ, 16)), -4.0, 4.0).astype(np.float32)
    other = synthetic.make_randomness(rng, STEPS, B, TV, prenet) + (np.clip(rng.normal(0.0, 1.5, (B, TQ, 16)), -4.0, 4.0).astype(np.float32),)
    return hp, weights.synthetic_weights(hp, seed=6), pad, tokens, tl, mels, ml, masks, noise, teacher, other


@pytest.mark.parametrize("forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_phase_calls_are_bitwise_the_whole_call(monkeypatch, name, forced):
    import torch
    from gst_tacotron_amd.model import GST_Tacotron
    hp, w, pad, tokens, tl, mels, ml, masks, noise, teacher, (masks2, noise2, teacher2) = _case(name)
    assert not np.array_equal(masks, masks2)
    monkeypatch.setenv("GSTTACO_PAD_DECODER", pad)
    gc.collect()
    m = GST_Tacotron(hyper_parameters=hp, max_batch=B, max_tokens=TV, max_ref_frames=TREF + 1)
    m.Restore(weights=w)
    how = dict(teacher_mels=teacher) if forced else dict(steps=STEPS)
    how2 = dict(teacher_mels=teacher2) if forced else dict(steps=STEPS)

    def randomness_is_the_injected():
        back_masks, back_noise = m.debug_randomness(STEPS, B, TV)
        assert back_masks.shape == masks.shape and np.array_equal(back_masks, masks)
        assert np.array_equal(back_noise, noise)

    for use in ("first use", "replay"):             # (with graphs, the default: the second round replays what the first captured)
        enc = m.encode(tokens)
        gst = m.Inference_GST_Step(mels, ml)
        m.decode(enc, gst, masks2, noise2, **how2)          # (leaves the other randomness / teacher in the workspace)
        mel, stop, _, align, pre = m.Inference_Step(tokens, tl, None, mels, ml, prenet_masks=masks, attn_noise=noise, return_pre_mel=True, **how)
        randomness_is_the_injected()
        other = m.Inference_Step(tokens, tl, None, mels, ml, prenet_masks=masks2, attn_noise=noise2, return_pre_mel=True, **how2)
        assert not torch.equal(other[4], pre)               # (the other randomness does change the frames)
        p_pre, p_stop, p_align = m.decode(enc, gst, masks, noise, **how)
        p_mel = m.postnet(p_pre)
        randomness_is_the_injected()
        torch.cuda.synchronize()
        assert mel.shape == (B, STEPS * R, 16) and stop.shape == (B, STEPS) and align.shape == (B, STEPS, TV)
        for what, a, b in (("mel", mel, p_mel), ("pre_mel", pre, p_pre), ("stop", stop, p_stop), ("alignments", align, p_align)):
            assert torch.isfinite(a).all(), (use, what)
            assert torch.equal(a, b), (use, what, float((a - b).abs().max()))
    assert m.graph_cache_size() > 0 and m.handoff_error() == 0
    m.synchronize()
