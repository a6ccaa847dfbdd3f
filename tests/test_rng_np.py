"""CPU: oracle/rng_np.py, the host restatement of the device random numbers (csrc/device_utils.h), against known answers and at
its edge values.  tests/test_gpu_rng.py and tests/test_gpu_audio.py then hold the device to it word for word."""
import numpy as np
import pytest

from oracle import rng_np as R

# Philox4x32-10 known answers, (key0, key1) / (c0, c1, c2, c3) -> output: the zero, all-ones and digits-of-pi vectors of the Random123
# distribution's known-answer set (its kat_vectors file lists counter, key, output).  They were written down from memory -- the published
# file was not at hand -- but a transcription that reproduces three 128-bit outputs, one of them keyed and countered with the hex digits
# of pi, is not a coincidence: the round function, its constants, the word order and the key schedule are pinned by them.
PHILOX_KAT = [
    ((0x00000000, 0x00000000), (0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("key,ctr,out", PHILOX_KAT)
def test_philox4x32_10_known_answers(key, ctr, out):
    got = R.philox4x32_10(key[0] | (key[1] << 32), *ctr)           # the seed's low word is key word 0
    assert tuple(int(v) for v in got) == out
    assert all(v.dtype == np.uint32 for v in got)


def test_philox_is_vectorised_and_every_argument_matters():
    """Arrays give what scalars give; each of the six input words changes the output (a swapped counter word or an ignored key
    word would show here before it shows on the device)."""
    key, ctr, out = PHILOX_KAT[2]
    seed = key[0] | (key[1] << 32)
    c0 = np.array([ctr[0], 0, 0xFFFFFFFF], np.uint32)
    got = R.philox4x32_10(seed, c0, ctr[1], ctr[2], ctr[3])
    assert got[0].shape == (3,) and tuple(int(v[0]) for v in got) == out
    assert tuple(int(v[1]) for v in got) == tuple(int(v) for v in R.philox4x32_10(seed, 0, ctr[1], ctr[2], ctr[3]))
    base = tuple(int(v) for v in R.philox4x32_10(seed, *ctr))
    seen = {base}
    for i in range(4):
        c = list(ctr)
        c[i] ^= 1
        seen.add(tuple(int(v) for v in R.philox4x32_10(seed, *c)))
    seen.add(tuple(int(v) for v in R.philox4x32_10(seed ^ 1, *ctr)))
    seen.add(tuple(int(v) for v in R.philox4x32_10(seed ^ (1 << 32), *ctr)))
    assert len(seen) == 7
    # a counter that is a permutation of another's words is a different counter
    assert tuple(int(v) for v in R.philox4x32_10(seed, ctr[1], ctr[0], ctr[2], ctr[3])) != base
    assert tuple(int(v) for v in R.philox4x32_10(seed, 5, 0, 0, 0x2000)) != tuple(int(v) for v in R.philox4x32_10(seed, 0, 5, 0, 0x2000))


def test_murmur3_finaliser_on_a_hand_computed_word():
    """fmix32(1), step by step: 1 ^ (1 >> 16) = 1; x 0x85EBCA6B = 0x85EBCA6B; ^ (>> 13 = 0x00042F5E) = 0x85EFE535;
    x 0xC2B2AE35 mod 2^32 = 0x514E79F9; ^ (>> 16 = 0x0000514E) = 0x514E28B7."""
    assert (0x85EBCA6B >> 13) == 0x00042F5E and (0x85EBCA6B ^ 0x00042F5E) == 0x85EFE535
    assert (0x85EFE535 * 0xC2B2AE35) & 0xFFFFFFFF == 0x514E79F9
    assert (0x514E79F9 ^ (0x514E79F9 >> 16)) == 0x514E28B7
    assert int(R.mix32(1)) == 0x514E28B7
    assert int(R.mix32(0)) == 0                                       # the finaliser's one fixed point
    assert [int(v) for v in R.mix32(np.array([1, 0], np.uint32))] == [0x514E28B7, 0]


def test_keep_word_chains_three_finalisers_over_both_seed_words():
    seed, step, layer, row, word = 0x9E3779B97F4A7C15, 3, 1, 2, 5
    h = int(R.mix32((seed & 0xFFFFFFFF) ^ ((step * 0x9E3779B1 + layer) & 0xFFFFFFFF)))
    h = int(R.mix32(h ^ (seed >> 32) ^ ((row * 0x85EBCA77) & 0xFFFFFFFF)))
    h = int(R.mix32(h ^ ((word * 0xC2B2AE3D + 0x27D4EB2F) & 0xFFFFFFFF)))
    assert int(R.keep_word(seed, step, layer, row, word)) == h
    others = {int(R.keep_word(*a)) for a in ((seed & 0xFFFFFFFF, step, layer, row, word), (seed, step + 1, layer, row, word),
                                             (seed, step, 0, row, word), (seed, step, layer, row + 1, word),
                                             (seed, step, layer, row, word + 1))}
    assert h not in others and len(others) == 5
    # drop_keep at rate 0.5 reads bit (col & 31) of word (col >> 5)
    cols = np.arange(256)
    bits = R.drop_keep(seed, step, layer, row, cols, 256, 0.5)
    words = R.keep_word(seed, step, layer, row, np.arange(8))
    assert bits.dtype == np.float32
    assert np.array_equal(bits, ((words[cols >> 5] >> (cols & 31).astype(np.uint32)) & 1).astype(np.float32))


def test_u01_range_ends():
    lo, hi = R.u01(0), R.u01(0xFFFFFFFF)
    assert lo.dtype == np.float32 and float(lo) == 2.0 ** -24 and float(hi) == 1.0             # (0, 1]: never 0, so log is finite
    assert float(R.u01(0xFF)) == 2.0 ** -24 and float(R.u01(0x100)) == 2.0 ** -23            # the low 8 bits are dropped
    assert float(R.u01(0x7FFFFFFF)) == 0.5


def test_normal_at_the_extreme_uniform_is_finite():
    """u1 = 2^-24, u2 = 1 -> sqrt(48 ln 2) cos(2 pi) = 5.768...: the bound of every sample the device can draw."""
    z = float(R.normal(0, 0xFFFFFFFF))
    print("normal at u1 = 2^-24:", z)
    assert np.isfinite(z) and abs(z - np.sqrt(48.0 * np.log(2.0))) < 1e-12 and abs(z - 5.77) < 0.01
    assert float(R.normal(0xFFFFFFFF, 0)) == 0.0                                                # u1 = 1: radius 0
    assert abs(float(R.normal(0, 0x7FFFFFFF)) + np.sqrt(48.0 * np.log(2.0))) < 1e-12          # u2 = 1/2: cos = -1 (a sine would give 0)


def test_tensor_builders_layouts_and_counters():
    seed, steps, B, Tv = 0x9E3779B97F4A7C15, 3, 2, 7
    m = R.masks(seed, steps, B, 64, 32, 0.25)
    assert m.shape == (steps, B * 96) and m.dtype == np.float32 and set(np.unique(m)) == {0.0, 1.0}
    # [steps][B * P0 | B * P1]; Philox counter (row * ncols + col, step, 0, 0x1000 + layer), keep = u01 > rate
    t, b, col = 2, 1, 17
    x0 = R.philox4x32_10(seed, b * 64 + col, t, 0, 0x1000)[0]
    x1 = R.philox4x32_10(seed, b * 32 + col, t, 0, 0x1001)[0]
    assert m[t, b * 64 + col] == float(R.u01(x0) > np.float32(0.25)) and m[t, B * 64 + b * 32 + col] == float(R.u01(x1) > np.float32(0.25))
    assert abs(R.masks(seed, 8, 4, 256, 256, 0.25).mean() - 0.75) < 0.02 and abs(R.masks(seed, 8, 4, 256, 256, 0.5).mean() - 0.5) < 0.02
    h = R.masks(seed, steps, B, 64, 32, 0.5)
    assert h[t, B * 64 + b * 32 + col] == float((int(R.keep_word(seed, t, 1, b, 0)) >> col) & 1)
    n = R.noise(seed, steps, B, Tv)
    x, y, _, _ = R.philox4x32_10(seed, 1 * Tv + 4, 2, 0, 0x2000)
    assert n.shape == (steps, B, Tv) and n.dtype == np.float64 and n[2, 1, 4] == float(R.normal(x, y))
    p = R.gl_phase(seed, 2, 3, 5)
    x = R.philox4x32_10(seed, (1 * 3 + 2) * 5 + 4, 0, 0, 0x4000)[0]
    assert p.shape == (2, 3, 5) and p.dtype == np.float32 and p[1, 2, 4] == np.float32(int(x) >> 8) * np.float32(2.0 ** -24)
    assert 0.0 <= p.min() and p.max() < 1.0
    # the seed's high word reaches every builder
    lo = seed & 0xFFFFFFFF
    assert not np.array_equal(m, R.masks(lo, steps, B, 64, 32, 0.25)) and not np.array_equal(h, R.masks(lo, steps, B, 64, 32, 0.5))
    assert not np.array_equal(n, R.noise(lo, steps, B, Tv)) and not np.array_equal(p, R.gl_phase(lo, 2, 3, 5))
