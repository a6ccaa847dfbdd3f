"""GPU: the device random numbers (csrc/device_utils.h: gt_philox, gt_u01, gt_normal, gt_keep_word, gt_drop_keep) as throughput
mode uses them -- the prenet keep masks and the SMA sigmoid noise of a decode -- against the host restatement oracle/rng_np.py, word
for word, under a seed whose high 32 bits are set.  tests/test_rng_np.py pins the restatement itself to Philox4x32-10's known answers.

The tensors come from ``debug_randomness``: at a Philox rate they are what gt_rng_fill_kernel wrote before the decode, at the hashed
rate 0.5 they are regenerated from the seed the decode used (the front kernels derive the same bits themselves;
test_gpu_parity.py::test_throughput_mode_randomness_matches_oracle shows the decode did use these tensors).
"""
import numpy as np
import pytest

from oracle import rng_np
from test_gpu_parity import _full_case, _model

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15           # every other seed of the suite is below 2^32: the key's high word is 0 there
B, TV, TREF, STEPS = 3, 24, 40, 4
# Box-Muller on the device's fast intrinsics (__logf, __cosf) against float64 on the same float32 uniforms: the maximum over the 288
# samples of the SMA cases below, measured on an MI355X (the same at rate 0.5 and 0.25: the noise stream does not depend on the rate),
# with max |noise| = 3.137.  NOISE_TOL is 4 x that.
NOISE_ERR_MEASURED = 1.113e-6
NOISE_TOL = 4 * NOISE_ERR_MEASURED
NOISE_BOUND = 5.8                   # sqrt(-2 ln 2^-24) = 5.768: no sample can be larger


def _draw(m, case, seed):
    import torch
    _, _, tokens, tl, mels, ml, _, _ = case
    m.Inference_Step(tokens, tl, None, mels, ml, seed=seed, steps=STEPS)
    torch.cuda.synchronize()
    return m.debug_randomness(STEPS, B, TV)


@pytest.mark.parametrize("att,rate", [("SMA", 0.5), ("SMA", 0.25), ("BMA", 0.5)])
def test_masks_and_noise_are_the_host_restatement(att, rate):
    """cfg2's decoder sizes (prenet 256 / 256), 3 utterances x 24 tokens, 4 steps.  Masks: bitwise rng_np.masks -- the counter hash at
    rate 0.5, Philox counter (row * 256 + col, step, 0, 0x1000 + layer) with keep = u01 > rate otherwise.  Noise (SMA): rng_np.noise,
    float64 Box-Muller on the same words; the device's __logf / __cosf are not bitwise that, so the bound is 4 x the error measured on
    an MI355X (measured 1.113e-6, bound 4.45e-6) -- small enough to catch a sine for the cosine, the [0, 1) interval or a swapped word, each of which moves samples by O(1).
    The seed's high word must count, and the same seed must give the same tensors."""
    case = _full_case(B, TV, TREF, STEPS, seed=61, att=att, rate=rate)
    m = _model(case[0], case[1], B, TV, TREF + 1)
    masks, noise = _draw(m, case, SEED)
    ref = rng_np.masks(SEED, STEPS, B, 256, 256, rate).reshape(STEPS, 2, B, 256)
    print(att, rate, "masks: keep fraction", float(masks.mean()), "; elements differing from the host restatement:", int((masks != ref).sum()))
    assert masks.shape == ref.shape and np.array_equal(masks, ref)
    sma = att == "SMA"
    if sma:
        nref = rng_np.noise(SEED, STEPS, B, TV)
        err = float(np.abs(noise.astype(np.float64) - nref).max())
        print(att, rate, "noise: max abs error against float64 Box-Muller", err, "; max |noise|", float(np.abs(noise).max()), "; bound", NOISE_TOL)
        assert np.isfinite(noise).all() and np.abs(noise).max() <= NOISE_BOUND
        assert err <= NOISE_TOL
    masks_lo, noise_lo = _draw(m, case, SEED & 0xFFFFFFFF)
    assert not np.array_equal(masks_lo, masks) and np.array_equal(masks_lo, rng_np.masks(SEED & 0xFFFFFFFF, STEPS, B, 256, 256, rate).reshape(ref.shape))
    masks_2, noise_2 = _draw(m, case, SEED)
    assert np.array_equal(masks_2, masks)
    if sma:
        assert not np.array_equal(noise_lo, noise) and np.array_equal(noise_2, noise)


def test_hashed_masks_of_a_padded_decoder_are_in_the_callers_columns():
    """Prenet 128 / 128 is zero-padded to 256 / 256 at finalize; ``debug_randomness`` hands the masks back in the caller's layout
    (gt_relayout_masks_kernel).  The hash of a keep bit does not depend on the row width, so they are rng_np.masks at the caller's 128
    columns, bitwise.  (No Philox rate here: its counter uses the padded width, an internal detail.)"""
    import gc
    from gst_tacotron_amd import synthetic, weights
    hp = synthetic.config_hp("cfg2")
    hp["Tacotron2"]["Decoder"]["Prenet"]["Size"] = [128, 128]
    hp["Max_Step"] = 80
    w = weights.synthetic_weights(hp, seed=21)
    rng = np.random.default_rng(62)
    tokens, tl = synthetic.make_tokens(rng, B, TV)
    mels, ml = synthetic.make_ref_mels(rng, B, TREF)
    gc.collect()
    m = _model(hp, w, B, TV, TREF + 1)
    masks, _ = _draw(m, (hp, w, tokens, tl, mels, ml, None, None), SEED)
    ref = rng_np.masks(SEED, STEPS, B, 128, 128, 0.5).reshape(STEPS, 2, B, 128)
    print("padded decoder: keep fraction", float(masks.mean()), "; elements differing from the host restatement:", int((masks != ref).sum()))
    assert masks.shape == ref.shape and np.array_equal(masks, ref)
