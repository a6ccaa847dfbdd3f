"""GPU tests of the vocoders' size surface (tests/vocoder_surface_cases.py): csrc/melgan.hip, hifigan.hip and waveglow.hip at the widths
where the waves of a workgroup take uneven numbers of items or idle, at the sizes where a plan halves its tile, at launches of exactly
the 163840 bytes of LDS a plan admits, and at WaveGlow's K chunks of 64 and 16.

1. Every row against the float64 restatement, row by row over the row's own length, to the module's own K times the row's e32; the
   plan the row reaches (tile, form, lds of every launch) is asserted from gsttaco_*_plan inside the test.
2. The header's bitwise promises on the uneven and the shrunk rows.  3. NaN beyond a row reaches no sample.
4. HiFi-GAN's 16-bit forms at widths whose LDS rows pad 48 -> 64, 80 -> 96, 112 -> 128: every launch alone, and the chain.

The bars are the sibling files', imported from them and unchanged.  The measured ratios stand in the docstrings and in EXPERIMENTS.md."""
import numpy as np
import pytest

import test_gpu_hifigan as THG
import test_gpu_hifigan_half as G
import test_gpu_melgan as TMG
import test_gpu_waveglow as TWG
import vocoder_cases as V
import vocoder_surface_cases as S
from vocoder_harness import Vocoder

pytestmark = pytest.mark.gpu

K = {"melgan": TMG.K, "hifigan": THG.K, "waveglow": TWG.K}      # 4, 8, 8: each module's own measured bar

_VOCODERS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_contexts():
    """Every context of this module lives for the module only (the persistent decode launch of later files needs to be the process's
    one live context)."""
    yield
    for v in _VOCODERS.values():
        v.close()
    _VOCODERS.clear()


def _vocoder(name, operands=None):
    """One vocoder per row and operand form, sized for the row, kept for the module."""
    r = S.ROWS[name]
    if (name, operands) not in _VOCODERS:
        _VOCODERS[name, operands] = Vocoder(r.module, r.case.cfg, r.case.weights, len(r.case.frames), r.case.T, operands=operands)
    return _VOCODERS[name, operands]


def _run(v, r, mel, frames=None, z=None, ld=None):
    if r.module == "waveglow":
        return v(mel, frames, z=z, sigma=r.case.sigma, ld=ld)
    return v(mel, frames, ld=ld)


def _z(r, rows=slice(None), samples=None):
    return r.case.z[rows, :samples] if r.module == "waveglow" else None


def _min_frames(r):
    return r.case.cfg.min_frames if r.module != "waveglow" else 1


def _assert_the_row_reaches_its_plan(v, r, operands="float32"):
    """tile, form and lds of every launch the library planned are the restated rule's, and the rule's plan holds what the row names"""
    stages = getattr(v.ctx, r.module + "_plan")()[2]
    rule = S.rule_plan(r.module, r.case.cfg, operands)
    got = [(s["kind"], s["channels"], s["tile"], s["form"], s["lds"]) for s in stages if s["kind"] != "flow"]
    if r.module == "waveglow":
        up, layer = rule
        want = [up] + [layer] * (r.case.cfg.n_flows * r.case.cfg.n_layers)
    else:
        want = rule
    assert got == [(s["kind"], s["channels"], s["tile"], s["form"], s["lds"]) for s in want], r.name
    assert set(r.reach) <= {(s["kind"], s["channels"], s["tile"], s["form"], s["items"]) for s in rule}, r.name
    if r.name in S.EXACT_BOUND:         # a launch at exactly the bytes the plan admits as the most: it must run, not be refused
        assert V.LDS_MAX in [s[4] for s in got], r.name


# ---------------------------------------------------------------------------------------------------- 1. every row against float64
@pytest.mark.parametrize("name", S.NAMES)
def test_every_row_equals_the_float64_restatement_row_by_row(name):
    """Largest device error over the row's rows / e32(row), measured on an MI355X.  MelGAN (bar 4): mg_96_48 1.40 (2.0e-6 / 1.5e-6),
    mg_160_80_48 1.36 (2.6e-6 / 1.9e-6), mg_320 1.28 (4.1e-6 / 3.2e-6), mg_112 1.83 (2.8e-6 / 1.5e-6), mg_shrunk 1.41 (3.2e-6 / 2.2e-6).
    HiFi-GAN (bar 8): hg_96 1.39 (2.3e-6 / 1.6e-6), hg_160 1.96 (2.6e-6 / 1.3e-6), hg_320 1.48 (2.7e-6 / 1.8e-6), hg_224 1.67 (2.0e-6 /
    1.2e-6), hg_shrunk 1.42 (1.1e-6 / 7.4e-7).  WaveGlow (bar 8): wg_c48 1.10 (9.6e-7 / 8.7e-7), wg_c80 1.83 (1.3e-6 / 7.3e-7), wg_c96 1.42
    (1.4e-6 / 9.8e-7), wg_c64 0.59 (1.0e-6 / 1.8e-6), wg_c128 2.04 (2.0e-6 / 9.9e-7), wg_win_1794 1.00 (2.5e-7 / 2.5e-7), wg_win_1793 0.93
    (2.1e-7 / 2.2e-7), wg_win_1985 1.31 (2.9e-7 / 2.2e-7).  Every row sits where the modules' own tables do (0.6 .. 2.1): uneven items,
    idle waves, halved tiles, the launches at exactly 163840 bytes, kc 64 / 16 and one workgroup a CU all ran clean."""
    r = S.ROWS[name]
    c = r.case
    want, want_len = S.reference(name)[:2]
    e32 = S.e32(name)
    v = _vocoder(name)
    _assert_the_row_reaches_its_plan(v, r)
    wav, lengths = _run(v, r, c.mel, c.frames_array, _z(r))
    assert np.array_equal(lengths, want_len)                    # lengths exactly
    assert np.isfinite(wav).all()
    if r.module != "waveglow":
        assert np.abs(wav).max() <= 1.0
    worst = 0.0
    for b, n in enumerate(want_len):
        assert not wav[b, n:].any(), (name, b)                  # zeros beyond the row, exactly; an empty row is all zeros
        if n:
            worst = max(worst, float(np.abs(wav[b, :n].astype(np.float64) - want[b, :n]).max()))
    print("surface row", name, "device error", worst, "e32", e32, "ratio", worst / e32, "bar", K[r.module])
    assert worst <= K[r.module] * e32
    assert (want_len == 0).sum() == sum(n < _min_frames(r) for n in c.frames) >= 1


# ---------------------------------------------------------------------------------------------------- 2. bitwise promises
@pytest.mark.parametrize("name", S.BITWISE)
def test_a_call_repeats_and_a_row_in_its_batch_is_the_row_alone(name):
    r = S.ROWS[name]
    c = r.case
    hop = c.cfg.hop
    v = _vocoder(name)
    wav, lengths = _run(v, r, c.mel, c.frames_array, _z(r))
    again, again_len = _run(v, r, c.mel, c.frames_array, _z(r))
    assert np.array_equal(wav, again) and np.array_equal(lengths, again_len)
    for b, n in enumerate(c.frames):
        if n >= _min_frames(r):
            alone, alone_len = _run(v, r, c.mel[b:b + 1, :n], None, _z(r, slice(b, b + 1), n * hop))      # B = 1, T = its frames, no lengths
            assert alone_len[0] == lengths[b] == n * hop and np.array_equal(alone[0], wav[b, :lengths[b]]), (name, b)
    wide, _ = _run(v, r, c.mel, c.frames_array, _z(r), ld=c.T * hop + 37)      # a wider wav: the same samples, zeros in the extra columns
    assert np.array_equal(wide[:, :wav.shape[1]], wav) and not wide[:, wav.shape[1]:].any()
    big = Vocoder(r.module, c.cfg, c.weights, len(c.frames), 2 * c.T)           # twice the capacity: other grids, the same bits
    try:
        got, got_len = _run(big, r, c.mel, c.frames_array, _z(r))
    finally:
        big.close()
    assert np.array_equal(got, wav) and np.array_equal(got_len, lengths)


# ---------------------------------------------------------------------------------------------------- 3. NaN beyond a row
@pytest.mark.parametrize("name", S.NAN_BEYOND)
def test_nan_beyond_a_row_reaches_no_sample(name):
    """With a halo wider than the tile (mg_shrunk, hg_shrunk) and waves that idle through a pass (all three), a bound taken at the tile
    instead of at the row reads what lies beyond the row: the mel beyond each row's frames is NaN (WaveGlow: z beyond its samples too),
    and the wav is bitwise that of the plain call."""
    r = S.ROWS[name]
    c = r.case
    v = _vocoder(name)
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    wav, lengths = _run(v, r, c.mel, c.frames_array, _z(r))
    mel, z = np.array(c.mel), None
    for b, n in enumerate(c.frames):
        mel[b, (n if n >= _min_frames(r) else 0):] = np.nan
    if r.module == "waveglow":
        z = np.array(c.z)
        for b, n in enumerate(c.frames):
            z[b, n * c.cfg.hop:] = np.nan
        assert np.isnan(z).any()
    assert np.isnan(mel).any() and np.abs(wav).max() > 0
    got, got_len = _run(v, r, mel, c.frames_array, z)
    assert np.array_equal(got_len, lengths) and np.array_equal(bits(got), bits(wav))
    for b, n in enumerate(lengths):
        assert not got[b, n:].any(), b


# ---------------------------------------------------------------------------------------------------- 4. HiFi-GAN's 16-bit forms
@pytest.mark.parametrize("precision", S.H.PRECISIONS)
@pytest.mark.parametrize("name", S.HALF)
def test_every_launch_alone_equals_its_float64_restatement_in_the_16_bit_forms(name, precision):
    """Every launch of the row's plan alone, through tests/test_gpu_hifigan_half.py's route and to its bar (8 x e32_launch).  Largest
    (device error / e32_launch) over the row's launches, measured on an MI355X, the same to every digit in bfloat16 and float16, so the
    largest is the one launch that does not depend on the form, the output conv (fp32 on the VALU in every form): hg_96 2.99 (16 launches), hg_160 2.59 (10), hg_224 2.84
    (5), hg_shrunk 2.91 (6, the d = 192 launch at exactly 163840 bytes of 16-bit rows among them)."""
    r = S.ROWS[name]
    c = r.case
    v = _vocoder(name, precision)
    _assert_the_row_reaches_its_plan(v, r, precision)
    plan = v.ctx.hifigan_plan()[2]
    ls = S.H.launches(c.cfg, c.weights)
    assert [(s["kind"], s["channels"], s["taps"], s["dilation"]) for s in plan] == [(l.kind, l.cout, l.taps, l.dil) for l in ls]
    rng = np.random.default_rng(100 + c.seed)
    worst, over = 0.0, []
    for i, l in enumerate(ls):
        err, e32 = G._run_one_launch(v, i, l, list(c.frames), rng, precision)
        assert e32 > 0
        worst = max(worst, err / e32)
        if err > G.K_LAUNCH * e32:
            over.append((i, l.kind, l.name, err, e32, err / e32))
    print("surface row", name, precision, "launches", len(ls), "largest launch error / e32_launch", worst)
    assert not over, over


@pytest.mark.parametrize("precision", S.H.PRECISIONS)
@pytest.mark.parametrize("name", S.HALF)
def test_the_16_bit_chain_stays_within_four_rounding_errors_of_exact_float64(name, precision):
    """Largest |device - exact float64| / e_h(row), bar 4 (tests/test_gpu_hifigan_half.py's), measured on an MI355X: bfloat16 hg_96
    1.00 (2.47e-2 / 2.47e-2), hg_160 1.00, hg_224 1.00, hg_shrunk 1.00; float16 hg_96 1.00 (3.11e-3 / 3.11e-3), hg_160 0.98, hg_224 1.00,
    hg_shrunk 1.00."""
    r = S.ROWS[name]
    c = r.case
    exact, want_len = S.reference(name)[:2]
    e_h = S.e_h(name, precision)
    wav, lengths = _vocoder(name, precision)(c.mel, c.frames_array)
    assert np.array_equal(lengths, want_len) and np.isfinite(wav).all() and np.abs(wav).max() <= 1.0
    worst = 0.0
    for b, n in enumerate(want_len):
        assert not wav[b, n:].any(), (name, b)
        if n:
            worst = max(worst, float(np.abs(wav[b, :n].astype(np.float64) - exact[b, :n]).max()))
    print("surface row", name, precision, "device - exact", worst, "e_h", e_h, "ratio", worst / e_h)
    assert worst <= G.K_CHAIN * e_h
    assert worst > 100 * S.e32(name)                            # and the 16-bit form really ran
