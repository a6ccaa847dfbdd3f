"""TEST INFRASTRUCTURE -- NumPy restatement of the device random numbers (csrc/device_utils.h: gt_philox, gt_u01, gt_normal,
gt_mix32, gt_keep_word, gt_drop_keep) and of the tensors the kernels build from them: the prenet keep masks and the SMA sigmoid
noise of throughput mode (csrc/attention.hip gt_rng_fill_kernel and every front kernel) and Griffin-Lim's initial phases
(csrc/audio.hip gt_gl_frames_kernel<INIT>).  Only tests/ may import this module.

Everything is integer arithmetic on uint32 / uint64 arrays (wrapping like the device's), so words, keep bits and the float32
uniforms are BITWISE what the device computes.  The one exception is ``normal``: the device evaluates Box-Muller with the fast
float32 intrinsics (__logf / __cosf); here it is float64 on the same float32 uniforms -- the reference value the device is
measured against, not a bit pattern.

Philox4x32-10 is the generator of Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11); the known
answers it is pinned to are in tests/test_rng_np.py.
"""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57           # multipliers of counter words 0 and 2
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85           # Weyl increments of the two key words
STREAM_PRENET0, STREAM_NOISE, STREAM_GL_PHASE = 0x1000, 0x2000, 0x4000      # 4th counter word
MASK32 = 0xFFFFFFFF


def _u32(x):
    """Any integer (array) reduced mod 2^32, as uint64 so that products do not overflow."""
    return np.asarray(x, dtype=np.uint64) & np.uint64(MASK32)


def philox4x32_10(seed, c0, c1, c2, c3):
    """gt_philox: key = (seed & 0xFFFFFFFF, seed >> 32), counter (c0, c1, c2, c3) -> four uint32 arrays (x, y, z, w)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & MASK32, seed >> 32
    c0, c1, c2, c3 = np.broadcast_arrays(_u32(c0), _u32(c1), _u32(c2), _u32(c3))
    m32, sh = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0                  # < 2^64: both factors are below 2^32
        p1 = np.uint64(PHILOX_M1) * c2
        n0 = (p1 >> sh) ^ c1 ^ np.uint64(k0)
        n1 = p1 & m32
        n2 = (p0 >> sh) ^ c3 ^ np.uint64(k1)
        n3 = p0 & m32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def u01(r):
    """gt_u01: (0, 1] in float32 from the top 24 bits -- ((r >> 8) + 1) * 2^-24, every step exact in float32."""
    r = np.asarray(r, dtype=np.uint32)
    return ((r >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)


def normal(r0, r1):
    """gt_normal: Box-Muller sqrt(-2 ln u1) cos(2 pi u2) on u1 = u01(r0), u2 = u01(r1), evaluated in float64."""
    u1, u2 = u01(r0).astype(np.float64), u01(r1).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def mix32(h):
    """gt_mix32: the murmur3 32-bit finaliser."""
    h = _u32(h)
    m32 = np.uint64(MASK32)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & m32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & m32
    h = h ^ (h >> np.uint64(16))
    return h


def keep_word(seed, step, layer, row, word):
    """gt_keep_word: the 32 keep bits of columns [32 word, 32 word + 32) -- three chained finalisers over (seed low, step, layer),
    (seed high, row), (word).  uint32 array."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    m32 = np.uint64(MASK32)
    lo, hi = np.uint64(seed & MASK32), np.uint64(seed >> 32)
    h = mix32(lo ^ ((_u32(step) * np.uint64(0x9E3779B1) + _u32(layer)) & m32))
    h = mix32(h ^ hi ^ ((_u32(row) * np.uint64(0x85EBCA77)) & m32))
    return mix32(h ^ ((_u32(word) * np.uint64(0xC2B2AE3D) + np.uint64(0x27D4EB2F)) & m32)).astype(np.uint32)


def drop_keep(seed, step, layer, row, col, ncols, rate):
    """gt_drop_keep: 1.0 keep / 0.0 drop (float32).  At rate 0.5 bit (col & 31) of keep_word(col >> 5); at any other rate Philox
    counter (row * ncols + col, step, 0, 0x1000 + layer), keep = u01(x) > rate compared in float32."""
    rate = np.float32(rate)
    col = _u32(col)
    if rate == np.float32(0.5):
        w = keep_word(seed, step, layer, row, col >> np.uint64(5)).astype(np.uint64)
        return ((w >> (col & np.uint64(31))) & np.uint64(1)).astype(np.float32)
    idx = (_u32(row) * _u32(ncols) + col) & np.uint64(MASK32)
    x = philox4x32_10(seed, idx, step, 0, _u32(layer) + np.uint64(STREAM_PRENET0))[0]
    return (u01(x) > rate).astype(np.float32)


def masks(seed, steps, B, P0, P1, rate):
    """The keep-mask tensor of a decode, in the C-ABI's flat layout [steps][B * P0 | B * P1] (float32 0 / 1)."""
    out = np.empty((steps, B * (P0 + P1)), np.float32)
    step = np.arange(steps)[:, None, None]
    for layer, (P, off) in enumerate(((P0, 0), (P1, B * P0))):
        row, col = np.arange(B)[None, :, None], np.arange(P)[None, None, :]
        out[:, off:off + B * P] = drop_keep(seed, step, layer, row, col, P, rate).reshape(steps, B * P)
    return out


def noise(seed, steps, B, Tv):
    """The SMA sigmoid noise of a decode [steps, B, Tv]: normal(x, y) of Philox counter (b * Tv + t, step, 0, 0x2000).  float64."""
    step = np.arange(steps)[:, None, None]
    idx = np.arange(B)[None, :, None] * Tv + np.arange(Tv)[None, None, :]
    x, y, _, _ = philox4x32_10(seed, idx, step, 0, STREAM_NOISE)
    return normal(x, y)


def gl_phase(seed, B, T, nb):
    """Griffin-Lim's initial phases / 2 pi [B, T, nb] in [0, 1): (x >> 8) * 2^-24 (float32, exact) of Philox counter
    ((b * T + t) * nb + k, 0, 0, 0x4000)."""
    idx = np.arange(B * T * nb, dtype=np.uint64).reshape(B, T, nb)
    x = philox4x32_10(seed, idx, 0, 0, STREAM_GL_PHASE)[0]
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
