"""The NumPy pieces the vocoders' float64 restatements share (tests/melgan_cases.py, hifigan_cases.py, waveglow_cases.py) and the
plans' rule, restated from its contract without a call into the library: the item form and time tile by channel count (``tile_form``,
csrc/vocoder_common.h), the LDS bytes of every launch kind, the halving of a tile that does not fit (``shrink``) and WaveGlow's K
chunk.  tests/test_vocoder_surface_cases.py holds the library's plans to it.  Every NumPy function keeps the dtype of its input."""
import numpy as np


def _leaky(x, slope):
    return np.where(x > 0, x, x * slope)


def _conv(x, w, b, taps, dil):
    """x [L, cin], w [taps * cin, cout] -> [L, cout], taps odd: zero padding (taps - 1) / 2 * dil each side; bias, then taps ascending"""
    cin = w.shape[0] // taps
    L, p = x.shape[0], (taps - 1) // 2 * dil
    xp = np.pad(x, ((p, p), (0, 0)))
    y = np.tile(b[None, :], (L, 1))
    for k in range(taps):
        y = y + xp[k * dil:k * dil + L] @ w[k * cin:(k + 1) * cin]
    return y


def _reflect(x, p):
    return np.pad(x, ((p, p), (0, 0)), mode="reflect")


def _transposed(x, w, b, r):
    """x [L, cin], w [2r, cin, cout]: output o = i r - r/2 + k, cropped to [0, r L): two taps per sample, nothing beyond the ends"""
    L = x.shape[0]
    full = np.zeros(((L + 1) * r, w.shape[2]), dtype=x.dtype)
    for k in range(2 * r):
        full[k:k + (L - 1) * r + 1:r] += x @ w[k]
    return full[r // 2:r // 2 + r * L] + b[None, :]


def _pad16(c):
    return (c + 15) // 16 * 16


def tile_form(n_p):
    """(time tile, N-tiles a wave item owns) of a launch of n_p padded output channels: the form by channel count, and the tile that
    gives four waves an item each"""
    ntiles = n_p // 16
    nt = 4 if ntiles % 4 == 0 and ntiles >= 16 else (2 if ntiles % 2 == 0 else 1)
    ngroups = ntiles // nt
    return 64 * (1 if ngroups >= 4 else 2 if ngroups >= 2 else 4), nt


LDS_MAX = 160 * 1024        # the dynamic LDS a workgroup of any vocoder launch may ask for; a plan admits lds <= LDS_MAX
ROWS, WAVES = 64, 4         # time rows of a wave item; waves of a workgroup


def _round32(c):
    return (c + 31) // 32 * 32


def row_bytes(cin_p, operands="float32"):
    """bytes of one staged LDS row of cin_p padded channels: cin_p + 4 floats, or round32(cin_p) + 8 halves in the 16-bit forms"""
    return (cin_p + 4) * 4 if operands == "float32" else (_round32(cin_p) + 8) * 2


def launch_lds(kind, tile, cin, taps=0, dil=0, operands="float32"):
    """LDS bytes of a MelGAN / HiFi-GAN launch of ``kind`` at time tile ``tile``; ``cin`` the unpadded input channels.  The output
    conv is fp32 in every operand form and has one tile."""
    if kind == "out":
        return ((256 + 6) * (cin | 1) + 7 * cin) * 4
    rows = {"in": tile + 6, "up": tile + 1, "res": 2 * tile + 2 * dil, "conv": tile + (taps - 1) * dil}[kind]
    return rows * row_bytes(_pad16(cin), operands)


def shrink(tile, lds_of):
    """The shrink rule of every plan: the tile halved from ``tile`` (tile_form's) while ``lds_of(tile)`` exceeds LDS_MAX and the tile
    is above one wave item's rows; None where the smallest tile does not fit (the plan refuses)."""
    while lds_of(tile) > LDS_MAX and tile > ROWS:
        tile //= 2
    return tile if lds_of(tile) <= LDS_MAX else None


def _mfma_launch(kind, cin, cout, rate, r=1, taps=0, dil=0):
    """One MelGAN / HiFi-GAN MFMA launch under the rule (float32 operands choose the tile), as a dict; None where it is refused.
    ``base_tile`` is tile_form's value, ``halo`` the rows staged beyond the tile, ``items`` the wave items of a workgroup."""
    n_p = _pad16(cout)
    base, form = tile_form(n_p)
    tile = shrink(base, lambda t: launch_lds(kind, t, cin, taps, dil))
    if tile is None:
        return None
    halo = {"in": 6, "up": 1, "res": 2 * dil, "conv": (taps - 1) * dil}[kind]
    return dict(kind=kind, channels=cout, cin=cin, taps=taps, dilation=dil, tile=tile, form=form, rate=rate, base_tile=base, halo=halo,
                ngroups=n_p // 16 // form, items=tile // ROWS * (n_p // 16 // form) * r, lds=launch_lds(kind, tile, cin, taps, dil))


def _out_launch(cin, rate):
    return dict(kind="out", channels=1, cin=cin, taps=7, dilation=1, tile=256, form=0, rate=rate, base_tile=256, halo=6, ngroups=0, items=0,
                lds=launch_lds("out", 256, cin))


def melgan_plan_rule(cfg):
    """What gsttaco_melgan_plan reports per launch, restated: a list of dicts (``rate`` is the rate of the launch's input for "up",
    of its output else, as the library reports it); None where the library refuses the configuration for its LDS."""
    ch, rate = cfg.channels(), 1
    out = [_mfma_launch("in", cfg.mel_dim, ch[0], 1)]
    for i, r in enumerate(cfg.ratios):
        out.append(_mfma_launch("up", ch[i], ch[i + 1], rate, r=r))
        rate *= r
        out += [_mfma_launch("res", ch[i + 1], ch[i + 1], rate, dil=3 ** j) for j in range(cfg.n_res)]
    out.append(_out_launch(ch[-1], rate))
    return None if any(s is None for s in out) else out


def hifigan_plan_rule(cfg, operands="float32"):
    """What gsttaco_hifigan_plan reports per launch, restated.  The tile is chosen with float32 operands;
    gsttaco_hifigan_set_operands recomputes ``lds`` alone at that tile."""
    ch, rate = cfg.channels(), 1
    out = [_mfma_launch("in", cfg.mel_dim, ch[0], 1, taps=7, dil=1)]
    for i, r in enumerate(cfg.rates):
        up = _mfma_launch("up", ch[i], ch[i + 1], rate, r=r)
        if up is not None:
            up.update(taps=2 * r, dilation=1)
        out.append(up)
        rate *= r
        for k, dils in zip(cfg.kernels, cfg.dilations):
            for d in dils:
                out.append(_mfma_launch("conv", ch[i + 1], ch[i + 1], rate, taps=k, dil=d))
                if cfg.resblock == 1:
                    out.append(_mfma_launch("conv", ch[i + 1], ch[i + 1], rate, taps=k, dil=1))
    out.append(_out_launch(ch[-1], rate))
    if any(s is None for s in out):
        return None
    if operands != "float32":
        for s in out:
            if s["kind"] != "out":
                taps, dil = (s["taps"], s["dilation"]) if s["kind"] == "conv" else (0, 0)
                s["lds"] = launch_lds(s["kind"], s["tile"], s["cin"], taps, dil, operands)
    return out


def waveglow_plan_rule(cfg):
    """The two MFMA launches of gsttaco_waveglow_plan, restated: {"up": ..., "layer": ...}; None where the library refuses the
    configuration for its LDS.  The upsampler takes tile_form's item form by mel_p and stages win / hop - 1 frames in front of its
    tile; the WN layer's gate GEMM owns ``form`` N-tiles (pairs of a tanh and a sigmoid tile) an item, and stages its K loop in chunks
    of ``kc``: the widest of 64, 32, 16 with which two workgroups share a CU's LDS (``share`` 2), else the widest that fits at all."""
    mel_p, C_p, back = _pad16(cfg.mel_dim), _pad16(cfg.n_channels), cfg.win // cfg.hop - 1
    base, form = tile_form(mel_p)
    up_lds = lambda t: (t + back) * (mel_p + 4) * 4
    tile = shrink(base, up_lds)
    if tile is None:
        return None
    up = dict(kind="up", channels=cfg.mel_dim, tile=tile, form=form, unit=cfg.hop, base_tile=base, halo=back, ngroups=mel_p // 16 // form,
              items=tile // ROWS * (mel_p // 16 // form) * cfg.hop, lds=up_lds(tile))
    pairs = C_p // 16
    form = 8 if pairs % 4 == 0 else 4 if pairs % 2 == 0 else 2
    ngroups = 2 * pairs // form
    tile = ROWS * (1 if ngroups >= 4 else 2 if ngroups >= 2 else 4)
    lds = lambda kc: tile * ((kc + 4) + (C_p + 4)) * 4
    chosen = [(kc, share) for share in (2, 1) for kc in (64, 32, 16) if share * lds(kc) <= LDS_MAX]
    if not chosen:
        return None
    kc, share = chosen[0]
    layer = dict(kind="layer", channels=cfg.n_channels, tile=tile, form=form, unit=cfg.n_group, ngroups=ngroups, items=tile // ROWS * ngroups,
                 kc=kc, share=share, C_p=C_p, lds=lds(kc))
    return dict(up=up, layer=layer)


def waveglow_kc_share(tile, C_p, lds):
    """(kc, share) of a WN layer launch, from the ``lds`` the library reports for it: lds = tile ((kc + 4) + (C_p + 4)) 4"""
    kc = lds // (4 * tile) - (C_p + 4) - 4
    assert kc in (16, 32, 64) and tile * ((kc + 4) + (C_p + 4)) * 4 == lds, (tile, C_p, lds)
    return kc, 2 if 2 * lds <= LDS_MAX else 1


def tile_edge_frames(tiles, min_frames=1):
    """One, zero and one more frame around the first and second multiple of each launch's time tile that a whole frame count
    reaches.  ``tiles``: rows that end in (tile, form, rate).  Frame counts below ``min_frames`` stay in (MelGAN's short rows must
    come out empty)."""
    frames = set()
    for *_, tile, _, rate in tiles:
        for m in (1, 2):
            if (m * tile) % rate == 0:
                f = m * tile // rate
                frames.update(v for v in (f - 1, f, f + 1) if v >= 1)
    return sorted(frames)
