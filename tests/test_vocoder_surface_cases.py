"""CPU checks of the vocoders' size surface (tests/vocoder_surface_cases.py): every row is admitted by the modules' own rule; the
library's plan -- gsttaco_{melgan,hifigan,waveglow}_configure + _plan straight through the C ABI, which needs no device -- equals the
rule restated in tests/vocoder_cases.py, for every row and for the three existing case tables; the table reaches every schedule
property it exists for, asserted from the rows' own plans; one step past an admitted row is refused by name and leaves the context
configurable; and two of the bugs the table exists for, put into the oracle, move the float64 result beyond the GPU test's bar."""
import numpy as np
import pytest

import hifigan_cases as HG
import melgan_cases as MG
import vocoder_cases as V
import vocoder_surface_cases as S
import waveglow_cases as WG
from gst_tacotron_amd import capi, synthetic

K_MELGAN = 4                    # tests/test_gpu_melgan.py's K: the bar the mutations must clear is K * e32(row)
TABLES = {"melgan": MG, "hifigan": HG, "waveglow": WG}


def _ctx():
    return capi.Context(synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4)


# ---------------------------------------------------------------------------------------------------- 1. admission
@pytest.mark.parametrize("name", S.NAMES)
def test_every_row_is_admitted(name):
    """Measured here, e32 / rms of the live samples: mg_96_48 1.5e-6 / 0.58, mg_160_80_48 1.9e-6 / 0.85, mg_320 3.2e-6 / 0.62, mg_112
    1.5e-6 / 0.68, mg_shrunk 2.2e-6 / 0.72; hg_96 1.6e-6 / 0.69, hg_160 1.3e-6 / 0.78, hg_320 1.8e-6 / 0.96, hg_224 1.2e-6 / 0.84,
    hg_shrunk 7.4e-7 / 0.74; wg_c48 8.7e-7 / 0.77, wg_c80 7.3e-7 / 0.73, wg_c96 9.8e-7 / 0.77, wg_c64 1.8e-6 / 0.74, wg_c128 9.9e-7 /
    0.79, wg_win_1794 2.5e-7 / 0.67, wg_win_1793 2.2e-7 / 0.59, wg_win_1985 2.2e-7 / 0.63 (max |s| of the WaveGlow rows: at most 1.13)."""
    r = S.ROWS[name]
    c = r.case
    out = S.reference(name)
    wav, lengths = out[:2]
    live = np.concatenate([wav[b, :lengths[b]] for b in range(len(c.frames))])
    rms, e32 = float(np.sqrt(np.mean(live * live))), S.e32(name)
    print("surface row", name, "e32", e32, "rms", rms, *(("max |s|", out[2]) if r.module == "waveglow" else ()))
    assert np.isfinite(wav).all() and np.isfinite(S.reference(name, "float32")[0]).all()
    assert e32 <= S.E32_MAX
    assert rms > S.RMS_MIN
    if r.module == "waveglow":
        assert out[2] <= S.SMAX
    else:
        assert np.abs(wav).max() <= 1.0
    min_frames = c.cfg.min_frames if r.module != "waveglow" else 1
    assert np.array_equal(lengths, [n * c.cfg.hop if n >= min_frames else 0 for n in c.frames])
    assert 0 in c.frames and max(c.frames) <= 200
    if r.module == "melgan":
        assert {min_frames - 1, min_frames} <= set(c.frames)
    for b, n in enumerate(lengths):
        assert not wav[b, n:].any()


@pytest.mark.parametrize("precision", S.H.PRECISIONS)
@pytest.mark.parametrize("name", S.HALF)
def test_the_16_bit_rows_are_admitted_by_their_rounding_error(name, precision):
    """e_h = max |rounded-operand float64 run - exact float64 run|, measured here: bfloat16 hg_96 2.5e-2, hg_160 2.1e-2, hg_224 1.1e-2,
    hg_shrunk 1.3e-2; float16 3.1e-3, 3.1e-3, 1.5e-3, 2.1e-3.  hifigan_half_cases' own bound, unchanged."""
    e_h = S.e_h(name, precision)
    print("surface row", name, precision, "e_h", e_h)
    assert 0 < e_h <= S.H.E_H_MAX[precision] and e_h > 100 * S.e32(name)


# ---------------------------------------------------------------------------------------------------- 2. the library's plan is the rule
def _library_plan(module, cfg, operands=None):
    """The MFMA and output launches gsttaco_*_plan reports, and for WaveGlow every launch; the context is closed again."""
    ctx = _ctx()
    try:
        getattr(ctx, module + "_configure")(cfg, 2, 8)
        if operands is not None:
            ctx.hifigan_set_operands(operands)
        return getattr(ctx, module + "_plan")()
    finally:
        ctx.close()


def _check_plan(module, cfg, operands=None):
    """The library's plan of ``cfg`` against the restated rule: kind, channels, tile, form, rate / unit and lds of every launch."""
    a, b, stages = _library_plan(module, cfg, operands)
    rule = S.rule_plan(module, cfg, operands or "float32")
    assert rule is not None and (a, b) == ((cfg.hop, cfg.n_group) if module == "waveglow" else (cfg.min_frames, cfg.hop))
    if module == "waveglow":
        up, layer = rule
        got_up = [s for s in stages if s["kind"] == "up"]
        got_layers = [s for s in stages if s["kind"] == "layer"]
        assert len(got_up) == 1 and len(got_layers) == cfg.n_flows * cfg.n_layers and stages[0]["kind"] == "up"
        fields = ("channels", "tile", "form", "unit", "lds")
        assert [got_up[0][f] for f in fields] == [up[f] for f in fields]
        for s in got_layers:
            assert [s[f] for f in fields] == [layer[f] for f in fields]
            assert V.waveglow_kc_share(s["tile"], layer["C_p"], s["lds"]) == (layer["kc"], layer["share"])
    else:
        fields = ("kind", "channels", "tile", "form", "rate", "lds") + (("taps", "dilation") if module == "hifigan" else ())
        assert [[s[f] for f in fields] for s in stages] == [[s[f] for f in fields] for s in rule]
    assert all(0 < s["lds"] <= V.LDS_MAX for s in stages)
    return rule


@pytest.mark.parametrize("name", S.NAMES)
def test_the_librarys_plan_of_every_row_is_the_restated_rule(name):
    r = S.ROWS[name]
    rule = _check_plan(r.module, r.case.cfg)
    reached = {(s["kind"], s["channels"], s["tile"], s["form"], s["items"]) for s in rule}
    assert set(r.reach) <= reached, (name, sorted(set(r.reach) - reached))
    if r.module == "hifigan":
        # gsttaco_hifigan_set_operands recomputes the bytes alone: the tile stays the one float32 operands chose, and still fits
        for precision in S.H.PRECISIONS:
            half = _check_plan("hifigan", r.case.cfg, precision)
            assert [s["tile"] for s in half] == [s["tile"] for s in rule] and all(h["lds"] <= f["lds"] for h, f in zip(half, rule))
        assert [s["lds"] for s in _check_plan("hifigan", r.case.cfg, "float32")] == [s["lds"] for s in rule]


@pytest.mark.parametrize("module", sorted(TABLES))
def test_the_existing_tables_go_through_the_rule_with_nothing_shrunk(module):
    """Every case of tests/{melgan,hifigan,waveglow}_cases.py: the library's plan is the rule's, no tile is below tile_form's, every
    MFMA launch has a multiple of four items, and WaveGlow's kc is 32 at two workgroups a CU -- what this table was added to leave."""
    M = TABLES[module]
    for name in M.NAMES:
        cfg = M.CASES[name].cfg
        rule = _check_plan(module, cfg)
        for s in rule:
            if s["kind"] != "out":
                assert s.get("base_tile", s["tile"]) == s["tile"] and s["items"] % V.WAVES == 0, (module, name, s)
            if s["kind"] == "layer":
                assert (s["kc"], s["share"]) == (32, 2), (name, s)
        if module == "hifigan":
            for precision in S.H.PRECISIONS:
                _check_plan(module, cfg, precision)


# ---------------------------------------------------------------------------------------------------- 3. what the table reaches
def _launches(module=None, kind=None):
    """(row name, launch) over the restated plans of the rows (pinned to the library's by the tests above), the output convs left out"""
    for name in S.NAMES:
        r = S.ROWS[name]
        if module in (None, r.module):
            for s in S.rule_plan(r):
                if s["kind"] != "out" and kind in (None, s["kind"]):
                    yield name, s


def test_the_table_reaches_every_schedule_it_exists_for():
    """Asserted from the rows' own plans, so that a later edit of a row cannot hollow the table out."""
    every = [s for _, s in _launches()]
    items = {s["items"] for s in every}
    reached = {
        "fewer items than waves: 3": 3 in items,
        "fewer items than waves: 1": 1 in items,
        "5 items": 5 in items, "6 items": 6 in items, "7 items": 7 in items,
        "form 4 with 5 groups": any(s["form"] == 4 and s["ngroups"] == 5 for s in every if s["kind"] != "layer"),
        "a halo wider than the tile": any(s.get("halo", 0) > s["tile"] for s in every),
        "kc 64": False, "kc 32": False, "kc 16": False, "share 1": False, "a partial last K chunk on hid": False,
    }
    for tag, module, kind in (("melgan res", "melgan", "res"), ("hifigan conv", "hifigan", "conv"), ("waveglow up", "waveglow", "up")):
        steps = {s["base_tile"] // s["tile"] for _, s in _launches(module, kind)}
        reached[tag + ": a tile unshrunk"] = 1 in steps
        reached[tag + ": a tile halved once"] = 2 in steps
        if tag != "melgan res":         # (MelGAN's 96 channels start at a tile of 128: one halving is all there is above 64)
            reached[tag + ": a tile halved twice"] = 4 in steps
    for module in ("hifigan", "waveglow"):
        reached[module + ": a launch at exactly the LDS bound"] = any(s["lds"] == V.LDS_MAX for _, s in _launches(module))
    for _, s in _launches("waveglow", "layer"):
        reached["kc %d" % s["kc"]] = True
        reached["share 1"] |= s["share"] == 1
        reached["a partial last K chunk on hid"] |= s["C_p"] > s["kc"] and s["C_p"] % s["kc"] != 0
    print("\n".join("%-50s %s" % (k, "reached" if v else "NOT REACHED") for k, v in reached.items()))
    assert all(reached.values()), [k for k, v in reached.items() if not v]
    # and the named rows are the ones that carry them
    lds = lambda name: [s["lds"] for s in S.rule_plan(S.ROWS[name]) if s["kind"] != "out"]
    assert all(V.LDS_MAX in lds(name) for name in S.EXACT_BOUND)
    for precision in S.H.PRECISIONS:    # hg_shrunk's d = 192 launch is at the bound in the 16-bit forms too
        assert V.LDS_MAX in [s["lds"] for s in S.rule_plan("hifigan", S.ROWS["hg_shrunk"].case.cfg, precision)]
    shrunk = S.rule_plan(S.ROWS["mg_shrunk"])[-2]
    assert (shrunk["kind"], shrunk["dilation"], shrunk["tile"], shrunk["base_tile"], shrunk["items"]) == ("res", 81, 64, 128, 3)
    assert S.ROWS["mg_shrunk"].case.cfg.min_frames == 41 and S.ROWS["mg_shrunk"].case.frames == (0, 40, 41, 64, 65, 97)
    assert set(S.BITWISE) | set(S.NAN_BEYOND) | set(S.HALF) | set(S.EXACT_BOUND) <= set(S.NAMES)
    # the 16-bit rows' widths pad their LDS rows past their channels by a remainder the existing tables never have
    pads = {(V._pad16(s["cin"]), V._round32(V._pad16(s["cin"]))) for n, s in _launches("hifigan") if n in S.HALF}
    assert {(48, 64), (80, 96), (112, 128)} <= pads


def test_hg_shrunk_straddles_its_dilations_and_its_tiles():
    c = S.ROWS["hg_shrunk"].case
    lens = {2 * n for n in c.frames}
    for d in (179, 192, 198):
        assert any(n < d for n in lens if n) and any(n > d for n in lens) and any(d <= n <= d + 2 for n in lens), d
    for tile in (64, 128, 256):
        assert {tile, tile + 2} <= lens
    convs = [s for s in S.rule_plan(S.ROWS["hg_shrunk"]) if s["kind"] == "conv"]
    assert [(s["dilation"], s["tile"], s["lds"], s["items"]) for s in convs] == [(179, 256, 163680, 4), (192, 128, 163840, 2), (198, 64, 163520, 1)]


# ---------------------------------------------------------------------------------------------------- 4. one step past a row
@pytest.mark.parametrize("module, cfg, field", S.REFUSED, ids=[m for m, _, _ in S.REFUSED])
def test_one_step_past_an_admitted_row_is_refused_by_name(module, cfg, field):
    assert S.rule_plan(module, cfg) is None                     # the rule refuses it too
    neighbour = S.ROWS[{"melgan": "mg_shrunk", "hifigan": "hg_shrunk", "waveglow": "wg_win_1985"}[module]].case.cfg
    ctx = _ctx()
    try:
        with pytest.raises(capi.GstTacoError) as e:
            getattr(ctx, module + "_configure")(cfg, 2, 8)
        assert e.value.code == -1 and field in str(e.value) and "LDS" in str(e.value), str(e.value)
        assert getattr(ctx, module + "_manifest")() == {}
        getattr(ctx, module + "_configure")(neighbour, 2, 8)    # the refusal left the context configurable: its admitted neighbour
        assert getattr(ctx, module + "_plan")()[2]
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------- 5. the bar sees these bugs
def test_the_bar_sees_a_skipped_item_and_a_reflection_at_the_tiles_end():
    """On mg_160_80_48's longest row, in float64: the input conv's fifth item skipped (five items for four waves: the one wave 0 takes
    in its second round), and block 1 of stage 0 (d = 3, tile 64) reflecting at its tile's end.  Measured here: the result moves by
    1.05 and 0.48, against a bar of 4 x 1.9e-6."""
    name = "mg_160_80_48"
    c = S.ROWS[name].case
    plan = S.rule_plan(S.ROWS[name])
    assert (plan[0]["kind"], plan[0]["tile"], plan[0]["form"], plan[0]["items"]) == ("in", 64, 2, 5)
    assert (plan[3]["kind"], plan[3]["dilation"], plan[3]["tile"]) == ("res", 3, 64)
    b = int(np.argmax(c.frames))
    x = c.mel[b, :c.frames[b]].astype(np.float64)
    assert c.frames[b] * c.cfg.ratios[0] > 2 * 64                # the row spans more than two tiles of that block
    want = MG.melgan_row(c.cfg, c.weights, x)
    assert np.array_equal(S.melgan_row_tiled(c.cfg, c.weights, x), want)
    assert np.array_equal(S.melgan_row_tiled(c.cfg, c.weights, x, res_reflect_at=(0, 1, 10 ** 6)), want)   # one tile: the row's end
    bar = K_MELGAN * S.e32(name)
    for tag, kw in (("skipped item", dict(skip_last_item_of_in=(64, 2))), ("reflection at the tile's end", dict(res_reflect_at=(0, 1, 64)))):
        moved = float(np.abs(S.melgan_row_tiled(c.cfg, c.weights, x, **kw) - want).max())
        print(tag, "moves the float64 result by", moved, "bar", bar)
        assert moved > 100 * bar
