"""GPU tests of the HiFi-GAN 16-bit operand forms at the edges of their operand types (tests/hifigan_edge_cases.py holds the tables;
tests/test_hifigan_edge_cases.py admits them on the CPU).

1. Selector probes: a launch whose kernel is a selector returns the device's rounded operand itself -- ties, the largest value,
   saturation, subnormals, zeros -- compared with ``==`` to the float32 restatement; the non-finite operands in a row of their own.
2. Weight probes: a delta activation returns the host's rounded weight through the MFMA's B operand, ``==`` again; a second pass
   lifts subnormal operands of either side by 2^10.
3. The float16 refusal at its boundary, 65520.
4. The real kernels of ``tiny``, ``odd_channels`` and ``halo`` inside float16's subnormal range and in its saturation, at the
   per-launch bar of tests/test_gpu_hifigan_half.py.
5. NaN beyond a row (per launch and in whole calls) and NaN in a neighbouring row.

What was measured on an MI355X stands in the docstrings below and in DESIGN 3.5."""
import numpy as np
import pytest

import hifigan_cases as M
import hifigan_edge_cases as E
import hifigan_half_cases as H
import test_gpu_hifigan_half as G

pytestmark = pytest.mark.gpu

FORMS = ("float32",) + H.PRECISIONS
NAN = float("nan")
_VOCODERS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_contexts():
    """Every context of this module lives for the module only (the persistent decode launch of later files needs to be the process's
    one live context)."""
    yield
    for v in _VOCODERS.values():
        v.close()
    _VOCODERS.clear()


def _kept(key, make):
    if key not in _VOCODERS:
        _VOCODERS[key] = make()
    return _VOCODERS[key]


def _case_vocoder(name, precision):
    c = M.CASES[name]
    return _kept(("case", name, precision), lambda: G._Vocoder(c.cfg, c.weights, len(c.frames) + 1, c.T, precision))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------- one launch on rows the test chose
def _inputs(l, frames, rng, draw=G._normal):
    """what tests/test_gpu_hifigan_half.py's harness draws for a launch, as a dict of rows"""
    ins = {"x": [draw(rng, (n * l.rate_in, l.cin)) for n in frames]}
    if l.res >= 0:
        ins["res"] = ins["x"] if l.res == l.src else [draw(rng, (n * l.rate_in, l.cout)) for n in frames]
    if l.sum == H.SUM_ADD:
        ins["sum"] = [draw(rng, (n * l.rate_in, l.cout)) for n in frames]
    return ins


def _launch(v, i, l, frames, ins, T, beyond=G.BEYOND):
    """Launch i of the plan alone on the rows ``ins`` at the call's T, every buffer and the mel holding ``beyond`` wherever no input
    was placed -> the rows' results as host arrays: [n * rate_out, C_p] with the padding channels, for the output conv [n * hop].
    Asserts that nothing outside the launch's output changed, by bits."""
    import torch
    cfg = v.cfg
    B = len(frames)
    assert B <= v.max_batch and max(frames) <= T <= v.max_frames
    wpf = H.ws_floats_per_frame(cfg)
    image = [torch.full((B * T * wpf,), beyond, dtype=torch.float32, device="cuda") for _ in range(4)]

    def place(buf, ch, data):
        cp = M._pad16(ch)
        for b, (n, a) in enumerate(zip(frames, data)):
            lo = b * T * l.rate_in * cp
            view = image[buf][lo:lo + n * l.rate_in * cp].view(n * l.rate_in, cp)
            view[:, :ch] = torch.as_tensor(np.array(a, dtype=np.float32)).cuda()
            view[:, ch:] = 0.0                      # the padding channels are exact zeros

    mel = torch.full((B, T, cfg.mel_dim), beyond, dtype=torch.float32, device="cuda")
    ld = T * cfg.hop
    wav = torch.full((B, ld), NAN, dtype=torch.float32, device="cuda")
    if l.kind == "in":
        for b, a in enumerate(ins["x"]):
            mel[b, :frames[b]] = torch.as_tensor(np.array(a, dtype=np.float32)).cuda()
    else:
        place(l.src, l.cin, ins["x"])
    if l.res >= 0 and l.res != l.src:
        place(l.res, l.cout, ins["res"])
    if l.sum == H.SUM_ADD:
        place(H.BUF_SUM, l.cout, ins["sum"])
    out_buf = None if l.kind == "out" else (H.BUF_SUM if l.sum != H.SUM_NONE else l.dst)
    fr = torch.as_tensor(np.asarray(frames, dtype=np.int32)).cuda()
    for k in range(4):
        v.buffer(k, image[k], True)
    v.stage(i, mel, fr, B, T, wav, ld)
    after = [torch.empty_like(image[k]) for k in range(4)]
    for k in range(4):
        v.buffer(k, after[k], False)
    torch.cuda.synchronize()
    expect = [t.clone() for t in image]
    rows = []
    if l.kind == "out":
        got = wav.cpu().numpy()
        for b, n in enumerate(frames):
            assert not got[b, n * cfg.hop:].any(), (i, b)                   # zeros beyond the row, up to ld_wav
            rows.append(got[b, :n * cfg.hop])
    else:
        cp = M._pad16(l.cout)
        for b, n in enumerate(frames):
            lo, size = b * T * l.rate_out * cp, n * l.rate_out * cp
            rows.append(after[out_buf][lo:lo + size].view(n * l.rate_out, cp).cpu().numpy())
            expect[out_buf][lo:lo + size] = after[out_buf][lo:lo + size]
    for k in range(4):
        assert torch.equal(after[k].view(torch.int32), expect[k].view(torch.int32)), ("launch", i, "wrote buffer", k, "outside its output")
    return rows


def _probe_vocoder(config, precision, tag, weights):
    cfg = E.PROBE_CFGS[config]
    return _kept(("probe", config, precision, tag), lambda: G._Vocoder(cfg, weights, 5, 272, precision))


def _paths(v, cfg, index):
    """(staging path, wave form) of a launch, from the plan"""
    s = v.ctx.hifigan_plan()[2][index]
    return ("scalar staging, no LeakyReLU" if s["kind"] == "in" else "vector staging, LeakyReLU"), s["form"], s["tile"]


# ---------------------------------------------------------------------------------------------------- 1. selector probes
@pytest.mark.parametrize("precision", H.PRECISIONS)
@pytest.mark.parametrize("config", tuple(E.PROBE_CFGS))
def test_a_selector_launch_returns_the_devices_rounded_operand(config, precision):
    """Measured on an MI355X, both forms, both configurations (narrow: form 1, tile 256 in all three launches; wide: form 2, tile 64
    in the input conv and 128 in the transposed conv and conv1): every asserted entry is ``==`` -- ties to even both ways and one
    float32 ulp beside them, the largest bfloat16, float16's saturation at 65504 from 65519.996, 65520, 1e6, FLT_MAX and inf, every
    float16 subnormal down to 2^-24 with the tie at 2^-25 to 0 and at 3 * 2^-25 to 2^-23, both signs -- through the scalar staging
    path (input conv) and the vector one behind the LeakyReLU (transposed conv, conv1).  Neither hg_cvt nor either MFMA flushes a
    subnormal operand: the pass at gain 2^10 returns 2^10 q for every subnormal q of both formats.  A float32-subnormal PRODUCT, 1.0 *
    a bfloat16 subnormal, is not asserted (the header does not speak of it); what the device returned is printed: exactly the
    product, every time (96 to 1 536 of them per launch, none as zero)."""
    cfg = E.PROBE_CFGS[config]
    T = max(E.FINITE_ROWS + (E.BAD_ROW,))
    for subnormals_only in (False, True):
        gain = E.GAIN if subnormals_only else 1.0
        v = _probe_vocoder(config, precision, ("selector", subnormals_only), E.selector_weights(cfg, gain))
        for index in E.PROBED:
            p = E.selector_probe(config, index, precision, subnormals_only)
            l = p["l"]
            print("hifigan selector probe", config, precision, "launch", index, l.kind, "gain", float(gain), "path / form / tile", _paths(v, cfg, index))
            rows = _launch(v, index, l, p["frames"], {"x": p["x"]}, T)
            flushed = kept = 0
            for b, n in enumerate(p["frames"]):
                got, want = rows[b][:, :l.cout], p["want"][b]
                assert not rows[b][:, l.cout:].any(), (index, b)                # the padding channels stay exact zeros
                ok = E.asserted(want)
                bad = ok & ~(got == want)
                assert not bad.any(), (config, precision, index, b, "first mismatches (device, want)",
                                       [(float(got[t, c]), float(want[t, c])) for t, c in zip(*np.nonzero(bad))][:8])
                flushed += int((got[~ok] == 0).sum())
                kept += int((got[~ok] == want[~ok]).sum())
            if not subnormals_only and precision == "bfloat16":
                print("hifigan selector probe", config, precision, "launch", index, "float32-subnormal products (not asserted): returned exactly",
                      kept, "returned as zero", flushed)
            if subnormals_only:
                continue
            # the non-finite operands, in a batch row of their own: that row is non-finite exactly where the restatement is, and the
            # other rows of the same call are bitwise what they are without it
            with_bad = _launch(v, index, l, p["frames"] + [E.BAD_ROW], {"x": p["x"] + [p["bad_x"]]}, T)
            for b in range(len(p["frames"])):
                assert np.array_equal(_bits(with_bad[b]), _bits(rows[b])), (index, b)
            got, want = with_bad[-1][:, :l.cout], p["bad_want"]
            finite = np.isfinite(want)
            assert np.array_equal(np.isfinite(got), finite) and np.array_equal(got[finite], want[finite]), (config, precision, index)


# ---------------------------------------------------------------------------------------------------- 2. weight probes
def _weight_probe_holds(v, config, index, precision, subnormals_only, weights=None):
    p = E.weight_probe(config, index, precision, subnormals_only, weights)
    l = p["l"]
    rows = _launch(v, index, l, p["frames"], {"x": p["x"]}, max(p["frames"]))
    flushed = kept = 0
    for b, n in enumerate(p["frames"]):
        got, want = rows[b][:, :l.cout], p["want"][b]
        assert not rows[b][:, l.cout:].any(), (index, b)
        ok = E.asserted(want)
        bad = ok & ~(got == want)
        assert not bad.any(), (config, precision, index, b, [(float(got[t, c]), float(want[t, c])) for t, c in zip(*np.nonzero(bad))][:8])
        flushed += int((got[~ok] == 0).sum())
        kept += int((got[~ok] == want[~ok]).sum())
    return rows, kept, flushed


@pytest.mark.parametrize("precision", H.PRECISIONS)
@pytest.mark.parametrize("config", tuple(E.PROBE_CFGS))
def test_a_delta_activation_returns_the_hosts_rounded_weight(config, precision):
    """Measured on an MI355X: every weight of the table comes back as ``round_operand(w)``, ``==``, tap by tap and channel by channel
    in all three launches of both configurations -- the host packers round as the header says (float16 subnormal weights
    2^-24 .. 2^-14 and nextafter(65520, 0) -> 65504 included), and neither MFMA flushes a subnormal B operand (amp 2^10 against the
    subnormal weights of both formats returns 2^10 q).  The float32-subnormal products of the bfloat16 pass at amp 1 are counted
    and printed, not asserted: 12 to 1 144 per launch, every one returned exactly, none as zero."""
    cfg = E.PROBE_CFGS[config]
    for subnormals_only in (False, True):
        v = _probe_vocoder(config, precision, ("weights", subnormals_only), E.probe_weights(config, precision, subnormals_only))
        for index in E.PROBED:
            _, kept, flushed = _weight_probe_holds(v, config, index, precision, subnormals_only)
            print("hifigan weight probe", config, precision, "launch", index, "amp", float(E.GAIN if subnormals_only else 1.0),
                  "path / form / tile", _paths(v, cfg, index), "float32-subnormal products (not asserted): returned exactly", kept, "as zero", flushed)


# ---------------------------------------------------------------------------------------------------- 3. the refusal boundary
def test_float16_refuses_exactly_65520_and_holds_the_float32_below_it():
    """65520 is the tie between 65504 and 65536 and rounds to even, so to inf: refused, at either sign, in the first and the last
    element of a tensor.  nextafter(65520, 0) finalizes and the weight probe reads 65504.  bfloat16 takes both (65520 -> 65536)."""
    config, cfg = "narrow", E.PROBE_CFGS["narrow"]
    below = np.nextafter(np.float32(65520.0), np.float32(0.0))
    names = [H.launches(cfg)[i].name + "/kernel" for i in E.PROBED]
    good = E.probe_weights(config, "float16")
    v = G._Vocoder(cfg, good, 3, 272, "float16", finalize=False)
    try:
        lib, h = v.ctx.lib, v.ctx.handle
        err = lambda: lib.gsttaco_last_error(h).decode()
        for name in names:
            for flat, value in ((0, 65520.0), (-1, -65520.0), (-1, 65520.0)):
                w = good[name].copy()
                w.reshape(-1)[flat] = value
                v.ctx.hifigan_load_weight(name, w)
                assert lib.gsttaco_hifigan_finalize(h) == -4 and name in err() and "float16" in err(), (name, flat, value)
            v.ctx.hifigan_load_weight(name, good[name])
        edge = {name: good[name].copy() for name in good}
        for name in names:
            edge[name].reshape(-1)[0], edge[name].reshape(-1)[-1] = below, -below
            v.ctx.hifigan_load_weight(name, edge[name])
        v.ctx.hifigan_finalize()
        for index in E.PROBED:
            rows, _, _ = _weight_probe_holds(v, config, index, "float16", False, edge)
            assert rows[0].max() == 65504.0 and rows[0].min() == -65504.0
    finally:
        v.close()
    for value in (65520.0, float(below)):
        w = {name: good[name].copy() for name in good}
        for name in names:
            w[name].reshape(-1)[0], w[name].reshape(-1)[-1] = value, -value
        b = G._Vocoder(cfg, w, 3, 272, "bfloat16")
        try:
            for index in E.PROBED:
                rows, _, _ = _weight_probe_holds(b, config, index, "bfloat16", False, w)
                assert rows[0].max() == 65536.0 and rows[0].min() == -65536.0
        finally:
            b.close()


# ---------------------------------------------------------------------------------------------------- 4. the real kernels at the ends of the range
@pytest.mark.parametrize("regime,precision", [(r, p) for r, (_, forms) in E.REGIMES.items() for p in forms])
@pytest.mark.parametrize("name", E.REGIME_CASES)
def test_every_launch_alone_holds_in_the_subnormal_range_and_in_saturation(name, regime, precision):
    """Largest (device error / e32_launch) over the case's launches, measured on an MI355X; the bar is the harness's own
    K_LAUNCH = 8.  small (N(0, 1) * 2^-15: about 97 % of the staged float16 operands are subnormals; a flush below 2^-14 would cost
    3 000 to 16 000 e32_launch, tests/test_hifigan_edge_cases.py): bfloat16 tiny 1.91, odd_channels 2.98, halo 1.98; float16 1.71,
    2.43, 1.95.  loud (N(0, 1) * 2^16, float16: about 16 % of the operands saturate): 1.18, 1.00, 1.12 (the output conv's tanh is
    exactly +-1 there in float32, float64 and on the device).  None is above 4: nothing to explain."""
    c = M.CASES[name]
    draw = E.REGIMES[regime][0]
    v = _case_vocoder(name, precision)
    plan = v.ctx.hifigan_plan()[2]
    ls = H.launches(c.cfg, c.weights)
    rng = np.random.default_rng(300 + c.seed)
    worst, over = 0.0, []
    for i, l in enumerate(ls):
        err, e32 = G._run_one_launch(v, i, l, G._launch_rows(name, plan[i]), rng, precision, draw=draw)
        # (loud: the output conv's tanh is exactly +-1 in float32 and float64 alike, e32_launch is 0 and the device must be exact too)
        assert e32 > 0 or (l.kind == "out" and regime == "loud"), (i, l.kind)
        worst = max(worst, err / e32 if e32 > 0 else 0.0)
        if err > G.K_LAUNCH * e32:
            over.append((i, l.kind, l.name, err, e32))
    print("hifigan", precision, "case", name, "regime", regime, "launches", len(ls), "largest launch error / e32_launch", worst)
    assert not over, over


# ---------------------------------------------------------------------------------------------------- 5. NaN as the sentinel
@pytest.mark.parametrize("precision", FORMS)
@pytest.mark.parametrize("name", E.REGIME_CASES)
def test_nan_beyond_a_row_reaches_no_launch(name, precision):
    """(a) Every launch alone with NaN in the mel and in all four workspace buffers beyond every row's length: finite results, bitwise
    those of the run with 1e3 there, nothing written outside the output.  A bound taken as a product, or a masked value discarded after
    an arithmetic step, passes with a finite filler and fails here."""
    c = M.CASES[name]
    v = _case_vocoder(name, precision)
    plan = v.ctx.hifigan_plan()[2]
    ls = H.launches(c.cfg, c.weights)
    for i, l in enumerate(ls):
        frames = G._launch_rows(name, plan[i])
        T = max(max(frames), 1)
        runs = [G._run_one_launch(v, i, l, frames, np.random.default_rng(400 + i), precision, beyond=b) for b in (G.BEYOND, NAN)]
        assert runs[0] == runs[1] and runs[1][0] <= G.K_LAUNCH * runs[1][1], (i, runs)
        ins = _inputs(l, frames, np.random.default_rng(400 + i))
        plain, nan = (_launch(v, i, l, frames, ins, T, beyond=b) for b in (G.BEYOND, NAN))
        for b, n in enumerate(frames):
            assert np.isfinite(nan[b]).all() and np.array_equal(_bits(nan[b]), _bits(plain[b])), (name, precision, i, b)


def _nan_beyond(mel, frames, min_frames=1):
    """the mel with NaN beyond each row's frames, and in the whole mel of a row too short to run"""
    out = np.array(mel, dtype=np.float32)
    for b, n in enumerate(frames):
        out[b, (n if n >= min_frames else 0):] = np.nan
    return out


@pytest.mark.parametrize("precision", FORMS)
@pytest.mark.parametrize("name", ["tiny", "halo"])
def test_nan_beyond_a_row_reaches_no_whole_call(name, precision):
    """(b) the free-run frames past the stop token are what sits beyond a row in Inference(..., vocoder=), and they may be NaN"""
    c = M.CASES[name]
    v = _case_vocoder(name, precision)
    wav, lengths = v(c.mel, c.frames_array)
    mel = _nan_beyond(c.mel, c.frames)
    assert np.isnan(mel).any() or min(c.frames) == c.T
    got, got_len = v(mel, c.frames_array)
    assert np.array_equal(got_len, lengths) and np.array_equal(_bits(got), _bits(wav))
    for b, n in enumerate(lengths):
        assert not got[b, n:].any(), (name, b)
    if name == "halo":              # every row of halo is long: cut them, so that NaN lies beyond each
        frames = np.maximum(c.frames_array - 2 * np.arange(len(c.frames)) - 1, 0).astype(np.int32)
        want, want_len = v(c.mel, frames)
        got, got_len = v(_nan_beyond(c.mel, frames), frames)
        assert np.array_equal(got_len, want_len) and np.array_equal(_bits(got), _bits(want)) and np.abs(want).max() > 0
        for b, n in enumerate(want_len):
            assert not got[b, n:].any(), (name, b)


@pytest.mark.parametrize("precision", FORMS)
@pytest.mark.parametrize("name", ["tiny", "halo"])
def test_a_row_of_nan_leaves_its_neighbours_bitwise_alone(name, precision):
    """(c) one row's mel is NaN inside its own length: every other row is bitwise the row run alone; the bad row holds whatever it
    holds up to its length and zeros beyond it."""
    c = M.CASES[name]
    v = _case_vocoder(name, precision)
    bad = int(np.argmax(c.frames_array >= 2))
    mel = c.mel.copy()
    mel[bad, c.frames[bad] // 2, 1] = np.nan
    frames = c.frames_array.copy()
    frames[bad] = c.frames[bad] - (1 if c.frames[bad] == c.T and name == "tiny" else 0)      # (tiny's bad row is the longest: leave room beyond it)
    wav, lengths = v(mel, frames)
    assert np.array_equal(lengths, frames * c.cfg.hop)
    assert not wav[bad, lengths[bad]:].any()
    for b, n in enumerate(frames):
        if b != bad:
            assert not wav[b, lengths[b]:].any()
            if n >= 1:
                alone, alone_len = v(c.mel[b:b + 1, :n])
                assert alone_len[0] == lengths[b] and np.array_equal(_bits(alone[0]), _bits(wav[b, :lengths[b]])), (name, precision, b)
