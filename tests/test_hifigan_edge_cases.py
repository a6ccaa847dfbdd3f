"""CPU tests of tests/hifigan_edge_cases.py: the tables and references of the HiFi-GAN 16-bit forms' edge probes are admitted here,
before tests/test_gpu_hifigan_edges.py holds the device to them with ``==``.  A probe whose restatement is not exact fails HERE."""
import numpy as np
import pytest

import hifigan_cases as M
import hifigan_edge_cases as E
import hifigan_half_cases as H
from gst_tacotron_amd import capi, hifigan, synthetic

CONFIGS = tuple(E.PROBE_CFGS)


def _same(a, b):
    """bitwise-in-value equality that lets NaN equal NaN (the sign of zero is not compared)"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("leaky", (False, True))
@pytest.mark.parametrize("precision", E.PRECISIONS)
def test_round_operand_gives_what_the_formats_definition_says_at_every_edge(precision, leaky):
    entries = E.edge_entries(precision, leaky)
    for cls, sign, x, want in entries:
        staged = E.leaky_f32(x) if leaky else x
        with np.errstate(invalid="ignore"):
            got = hifigan.round_operand(np.float32(staged), precision)
        assert got.dtype == np.float32 and _same(got, want), (cls, sign, x, got, want)
        if leaky and sign < 0 and cls not in ("saturated", "overflow"):
            # the negative x was chosen so that the slope's float32 image IS the edge: the positive entry of the same class, negated
            assert any(c == cls and s > 0 and staged == -px for c, s, px, _ in entries), (cls, x, staged)
    classes = {c for c, s, _, _ in entries if s > 0}
    assert classes >= {"tie_down", "tie_up", "beside_tie", "largest", "subnormal", "tie_to_zero", "subnormal_tie", "nan", "zero"}
    assert ("overflow" if precision == "bfloat16" else "saturated") in classes
    negative = {c for c, s, _, _ in entries if s < 0}
    assert negative >= set(E.NEGATIVE_BEHIND_THE_SLOPE[precision]) if leaky else negative == classes - {"nan"}
    # float16: every value the issue names is there
    if precision == "float16":
        xs = [float(x) for _, s, x, _ in entries if s > 0 and np.isfinite(x)]
        for v in (65504.0, float(np.nextafter(np.float32(65520), np.float32(0))), 65520.0, 1e6, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -24,
                  2.0 ** -25, float(np.nextafter(np.float32(2.0 ** -25), np.float32(1))), 3 * 2.0 ** -25):
            assert float(np.float32(v)) in xs, v


def test_the_slopes_preimage_is_exact_or_absent():
    for target in (-1.00390625, -2.0 ** -24, -3 * 2.0 ** -25, -2.0 ** -133, -2.0 ** -134, -1.0 - 2.0 ** -11):
        x = E.slope_preimage(target)
        assert x is not None and x < 0 and np.float32(x * np.float32(0.1)) == np.float32(target)
    assert E.slope_preimage(-np.inf) == -np.inf and E.slope_preimage(-0.0) == 0
    assert E.slope_preimage(-E.BF16_MAX) is None                       # ten times the largest bfloat16 is no float32


# ---------------------------------------------------------------------------------------------------- 1. selector probes
@pytest.mark.parametrize("subnormals_only", (False, True))
@pytest.mark.parametrize("precision", E.PRECISIONS)
@pytest.mark.parametrize("index", E.PROBED)
@pytest.mark.parametrize("config", CONFIGS)
def test_a_selector_launch_returns_the_rounded_operand_itself(config, index, precision, subnormals_only):
    p = E.selector_probe(config, index, precision, subnormals_only)
    l = p["l"]
    assert (l.kind == "in") == (not p["leaky"]) and not np.asarray(l.bias).any()
    with np.errstate(invalid="ignore"):
        want64 = H.launch_reference(l, {"x": [x.astype(np.float64) for x in p["x"]]}, p["frames"], precision, np.float64)
    seen = set()
    for b, n in enumerate(p["frames"]):
        x, want = p["x"][b], p["want"][b]
        assert want.dtype == np.float32 and x.shape == (n * l.rate_in, l.cin)
        if n == 0:
            assert want.shape == (0, l.cout)
            continue
        staged = E.leaky_f32(x) if p["leaky"] else x
        q = hifigan.round_operand(staged, precision)
        assert np.isfinite(q).all()
        assert np.array_equal(want, p["gain"] * E.place_selected(l, q))          # the restatement IS the operand, placed
        # float32 and float64 runs agree wherever the LeakyReLU's slope is not in play
        plus = E.place_selected(l, (x >= 0).astype(np.float32)) > 0
        assert plus.any() and np.array_equal(want64[b][plus], want[plus].astype(np.float64))
        # every entry of the table visits every channel of the row
        for cls, sign, ex, ew in p["entries"]:
            hits = x.view(np.int32) == np.float32(ex).view(np.int32)
            assert hits.any(axis=0).all(), (cls, sign, ex, b)
            if hits[:, :min(l.cin, l.cout)].any():
                seen.add((cls, sign))
            assert (want == p["gain"] * ew).any() or (ew == 0), (cls, sign, ex)
        if subnormals_only:
            assert E.is_subnormal16(q, precision).mean() > 0.5 and E.asserted(want).all()
        elif precision == "float16":
            assert E.asserted(want).all()                                            # 1.0 * a float16 subnormal is float32-normal
        else:
            assert not E.asserted(want).all() and E.asserted(want).mean() > 0.9      # 1.0 * a bfloat16 subnormal is not
    # every class is there after rounding, with both signs where the table has them
    assert seen == {(c, s) for c, s, _, _ in p["entries"]}
    if not subnormals_only:
        assert {c for c, _ in seen} >= {"tie_down", "tie_up", "beside_tie", "largest", "subnormal", "tie_to_zero", "subnormal_tie", "zero"}
    # the row of the non-finite operands: non-finite exactly where a tap of the window holds one (0 * inf = NaN: all channels)
    bad_q = hifigan.round_operand(E.leaky_f32(p["bad_x"]) if p["leaky"] else p["bad_x"], precision)
    hit = ~np.isfinite(bad_q).all(axis=1)
    assert hit.sum() == len(p["bad_entries"]) >= 1 and {c for c, _, _, _ in p["bad_entries"]} >= {"nan"}
    if l.kind == "up":              # position i feeds the 2 r samples from i r - r / 2 on, through a selector or through a zero
        window = np.zeros(len(hit) * l.r, dtype=bool)
        for i in np.nonzero(hit)[0]:
            window[max(i * l.r - l.r // 2, 0):i * l.r - l.r // 2 + 2 * l.r] = True
    else:                           # dilation 1: the taps around a sample
        window = np.convolve(hit.astype(int), np.ones(l.taps, dtype=int), mode="same") > 0
    mask = ~np.isfinite(p["bad_want"])
    assert np.array_equal(mask, np.repeat(window[:, None], l.cout, axis=1)) and mask.any() and not mask.all()


# ---------------------------------------------------------------------------------------------------- 2. weight probes
@pytest.mark.parametrize("subnormals_only", (False, True))
@pytest.mark.parametrize("precision", E.PRECISIONS)
@pytest.mark.parametrize("index", E.PROBED)
@pytest.mark.parametrize("config", CONFIGS)
def test_a_delta_activation_returns_the_rounded_weight_itself(config, index, precision, subnormals_only):
    p = E.weight_probe(config, index, precision, subnormals_only)
    l, table = p["l"], E.weight_table(precision, subnormals_only)
    kernel = np.asarray(l.kernel)
    q = hifigan.round_operand(kernel, precision)
    assert np.isfinite(q).all()
    if precision == "float16":
        assert np.array_equal(q, kernel.astype(np.float16).astype(np.float32))                         # no weight saturates
    assert set(table.view(np.int32).tolist()) == set(kernel.view(np.int32).reshape(-1).tolist())       # every entry is in the kernel
    assert not np.asarray(l.bias).any()
    ones = np.ones_like(q)
    for b, n in enumerate(p["frames"]):
        x, want = p["x"][b], p["want"][b]
        if n == 0:
            continue
        assert set(np.unique(x).tolist()) == {0.0, float(p["amp"])}
        assert E.place_weights(l, (x != 0).astype(np.float32), ones).max() == 1.0      # every output sample is ONE product
        assert np.array_equal(want, E.place_weights(l, x, q))
        if subnormals_only or precision == "float16":
            assert E.asserted(want).all()
    if subnormals_only:
        assert E.is_subnormal16(q, precision).mean() > 0.9 and (p["amp"] == E.GAIN)
    # the full row reads every element of the kernel: the whole rounded table comes back
    back = set(np.unique(np.abs(p["want"][0])).tolist()) | {0.0}
    assert back == set(np.unique(np.abs(p["amp"] * q)).tolist()) | {0.0}
    if precision == "float16" and not subnormals_only:
        qs = set(np.unique(q).tolist())
        assert {65504.0, -65504.0, 2.0 ** -24, 2.0 ** -23, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14} <= qs
        assert np.nextafter(np.float32(65520), np.float32(0)) in table and 65520.0 not in table and not np.isinf(table).any()
        assert E.is_subnormal16(q, precision).sum() >= 20


# ---------------------------------------------------------------------------------------------------- 3. the refusal boundary, host side
def test_float16_refuses_a_weight_of_exactly_65520_before_any_device_is_touched():
    """The pack runs on the host ahead of every upload, so the refusal itself needs no device (the finalize that succeeds does:
    tests/test_gpu_hifigan_edges.py)."""
    cfg = E.PROBE_CFGS["narrow"]
    good = E.probe_weights("narrow", "float16")
    ctx = capi.Context(synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4)
    try:
        ctx.hifigan_configure(cfg, 2, 16)
        ctx.hifigan_set_operands("float16")
        ctx.hifigan_load_weights(good)
        err = lambda: ctx.lib.gsttaco_last_error(ctx.handle).decode()
        for i in E.PROBED:
            name = H.launches(cfg)[i].name + "/kernel"
            for flat, value in ((0, 65520.0), (-1, -65520.0)):
                w = good[name].copy()
                w.reshape(-1)[flat] = value
                ctx.hifigan_load_weight(name, w)
                assert ctx.lib.gsttaco_hifigan_finalize(ctx.handle) == -4 and name in err() and "float16" in err(), (name, flat)
            ctx.hifigan_load_weight(name, good[name])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------- 4. the regimes
def _staged(name, draw, precision):
    """the operands a case's residual convs stage from ``draw``: q(L(x)), one array"""
    c = M.CASES[name]
    rng = np.random.default_rng(500 + c.seed)
    x = draw(rng, (4096, c.cfg.channels()[1]))
    return hifigan.round_operand(E.leaky_f32(x), precision)


@pytest.mark.parametrize("name", E.REGIME_CASES)
def test_the_small_regime_is_float16s_subnormal_range_and_the_loud_one_saturates(name):
    q = _staged(name, E.draw_small, "float16")
    share = E.is_subnormal16(q, "float16").sum() / (q != 0).sum()
    assert share >= 0.90 and (q != 0).mean() > 0.9                     # by the normal tail about 97 % are
    q = _staged(name, E.draw_loud, "float16")
    sat = (np.abs(q) == 65504.0).mean()
    assert sat >= 0.10                                                  # about 16 % do
    print("hifigan regimes, case", name, "subnormal share", share, "saturated share", sat)
    assert set(E.REGIMES) == {"small", "loud"} and E.REGIMES["small"][1] == E.PRECISIONS and E.REGIMES["loud"][1] == ("float16",)


@pytest.mark.parametrize("precision", E.PRECISIONS)
@pytest.mark.parametrize("name", E.REGIME_CASES)
def test_a_flush_of_float16_subnormals_would_miss_the_small_regimes_bar(name, precision, monkeypatch):
    """The reason the small regime is run: with operands flushed below 2^-14 (what earlier matrix pipes did to float16 and, for the
    bfloat16 form, what a float16-style flush in the conversion would do) a residual conv of the case misses 8 e32_launch, the GPU
    test's bar, by more than a factor of ten."""
    c = M.CASES[name]
    l = next(l for l in H.launches(c.cfg, c.weights) if l.kind == "conv")
    frames = [n for n in c.frames if n >= 1][:2]
    rng = np.random.default_rng(300 + c.seed)
    ins = {"x": [E.draw_small(rng, (n * l.rate_in, l.cin)) for n in frames]}
    if l.res >= 0:
        ins["res"] = ins["x"]
    want = H.launch_reference(l, ins, frames, precision, np.float64)
    want32 = H.launch_reference(l, ins, frames, precision, np.float32)
    e32 = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(want32, want))
    plain = hifigan.round_operand
    monkeypatch.setattr(hifigan, "round_operand", lambda x, p: np.where(np.abs(plain(x, p)) < 2.0 ** -14, 0.0, plain(x, p)).astype(np.asarray(x).dtype))
    flushed = H.launch_reference(l, ins, frames, precision, np.float32)
    err = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(flushed, want))
    print("hifigan", precision, "case", name, "a flush would cost", err, "e32_launch", e32, "ratio", err / e32)
    assert e32 > 0 and err > 10 * 8 * e32
