"""CPU: the table of tests/decoder_surface_cases.py is sound (no GPU involved: these are properties of the rows, of the two oracles, of
the manifests and of gsttaco_create, not of the kernels)."""
import os
import re

import numpy as np
import pytest

import decoder_surface_cases as D
from gst_tacotron_amd import hparams, weights
from oracle import oracle_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKED = [(c.name, s) for c in D.CASES if c.lengths for s in c.lengths]
MIXED = [(c.name, s) for c in D.CASES if c.mixed for s in c.shapes]
FORCED = [(c.name, s) for c in D.CASES if c.forced for s in c.shapes]
ORACLE_BAR = 1e-9           # oracle/gen_golden.py's own bar between the two oracles


def _id(v):
    return v if isinstance(v, str) else "x".join(map(str, v))


def _dims(c):
    return hparams.Dims(D.hp_case(**c.hp))


def _padded(c):
    """pad_decoder's rule (csrc/gsttaco.cpp): every size at most the reference's and not all equal to it."""
    d = _dims(c)
    sizes = (d.prenet[0], d.prenet[1], d.att, d.dec_rnn[0], d.dec_rnn[1])
    ref = D.SHIPPED["prenet"] + (D.SHIPPED["att"],) + D.SHIPPED["rnn"]
    return all(s <= r for s, r in zip(sizes, ref)) and sizes != ref


def _reference_sized(c):
    d = _dims(c)
    return _padded(c) or (tuple(d.prenet), d.att, tuple(d.dec_rnn)) == (D.SHIPPED["prenet"], D.SHIPPED["att"], D.SHIPPED["rnn"])


# ---------------------------------------------------------------------------------------------------- admission
@pytest.mark.parametrize("name,shape", D.CALLS + [(n + "/masked", s) for n, s in MASKED] + [(n + "/forced", s) for n, s in FORCED], ids=_id)
def test_rows_are_admitted_by_the_oracle_alone(name, shape):
    """8 x the float32 floor is at most TOL on every output: the GPU bound is TOL on every row.  A row that fails here is replaced,
    never widened."""
    name, _, mode = name.partition("/")
    r = D.reference(name, shape, mode == "masked", mode == "forced")
    print(name, shape, mode, "float32 oracle against float64:", {k: "%.3g" % v for k, v in r.floor.items()},
          "scale", {k: "%.3g" % v for k, v in r.scale.items()})
    B, Tv, steps = shape
    d = _dims(D.BY_NAME[name])
    assert r.ref["mel"].shape == r.ref["pre_mel"].shape == (B, steps * d.r, d.mel)
    assert r.ref["stop"].shape == (B, steps) and r.ref["align"].shape == (B, steps, Tv)
    for k in D.OUTPUTS:
        assert np.isfinite(r.ref[k]).all() and r.scale[k] > 0.01, k
        assert D.FLOOR_FACTOR * r.floor[k] <= D.TOL, (k, r.floor[k])


@pytest.mark.parametrize("name,shape", MIXED, ids=_id)
def test_mixed_rows_are_real(name, shape):
    """The float64 and float32 evaluations of the bf16 emulation agree within drift / 16 on every output of the decode loop, in the
    mean norm the GPU test compares them in (the module's docstring says why not the maximum; both are printed)."""
    m = D.mixed_reference(name, shape)
    for k in D.OUTPUTS:
        print("%s %s %s: mean drift %.3g spread %.3g (x%.0f) GPU bound %.3g | max drift %.3g spread %.3g (x%.1f)%s" % (
            name, shape, k, m.drift[k], m.spread[k], m.drift[k] / m.spread[k], D.mixed_tolerance(m.drift[k]), m.drift_max[k], m.spread_max[k],
            m.drift_max[k] / m.spread_max[k], ", conditioned in the max norm too" if D.max_norm_conditioned(m, k) else ""))
        assert np.isfinite(m.ref[k]).all()
    for k in D.LOOP_OUTPUTS:
        assert m.spread[k] <= m.drift[k] / 16, k
        assert D.mixed_tolerance(m.drift[k]) > 8 * D.reference(name, shape).floor[k]       # (the bound leaves room for fp32 noise)
    for k in D.OUTPUTS:
        assert m.drift_max[k] < D.MIXED_TOL         # (the suite's max-norm bar leaves room above the mode's own distance from fp32)


# ---------------------------------------------------------------------------------------------------- the two oracles agree
@pytest.mark.parametrize("name,shape", [("p112x9", (32, 17, 6)), ("p128x5_gst", (17, 19, 6))], ids=_id)
def test_oracles_agree_in_float64(name, shape):
    """oracle_np against oracle/torch_ref.py (the Value projection not hoisted, concat-grown loop state, torch's own conv1d and LSTM
    cell) on a row with r = 9 and on the GST row, unequal prenet sizes in both: the masks go in per layer."""
    import torch
    from oracle.torch_ref import TorchReference
    hp, w = D.model_of(name)
    assert name != "p112x9" or hp["Step_Reduction"] == 9
    x = D.inputs(name, shape)
    tr = TorchReference(hp, {k: np.array(v) for k, v in w.items()}, dtype=torch.float64)      # (writable copies: torch wants them)
    with torch.no_grad():
        memory = tr.encoder(np.array(x.tokens))
        if hp["GST"]["Use"]:
            gst = tr.style_token_layer(torch.as_tensor(np.asarray(x.mels, np.float64)), x.mel_lengths)
            memory = torch.cat([gst.unsqueeze(1).repeat(1, memory.shape[1], 1), memory], dim=-1)
        masks = [tuple(torch.as_tensor(m) for m in ms) for ms in D.split_masks(hp, x.masks, shape[0])]
        pre, mel, stop, align = tr.decoder(memory, masks, torch.as_tensor(np.asarray(x.noise, np.float64)), shape[2])
    got = {"mel": mel.numpy(), "stop": stop.numpy(), "align": align.numpy(), "pre_mel": pre.numpy()}
    e = D.errs(got, D.reference(name, shape).ref)
    print(name, shape, "oracle_np against torch_ref, float64:", e)
    assert max(e.values()) <= ORACLE_BAR


def test_flat_masks_are_the_stacked_tensor_where_the_sizes_are_equal():
    """The flat layout is what every other test injects as [steps, 2, B, P]: oracle_np.inference_step on the stacked tensor is run_oracle."""
    name, shape = "att144", (5, 21, 6)
    hp, w = D.model_of(name)
    x = D.inputs(name, shape)
    mel, stop, _, align, inter = oracle_np.inference_step(hp, w, x.tokens, None, None, D.stacked_masks(hp, x.masks, shape[0]), x.noise,
                                                          steps=shape[2], dt=np.float64)
    e = D.errs({"mel": mel, "stop": stop, "align": align, "pre_mel": inter["pre_mel"]}, D.reference(name, shape).ref)
    assert max(e.values()) == 0.0, e


# ---------------------------------------------------------------------------------------------------- coverage of the table itself
def test_table_covers_the_branches_it_claims():
    by = D.BY_NAME
    for c in D.CASES:
        d = _dims(c)
        for s in c.shapes:
            assert 6 <= s[2] <= 10 and s[1] <= 40 and set(c.plan) == set(c.shapes)
            assert c.plan[s]["dec_padded"] == int(_padded(c)), c.name
            if "pj_tiles" in c.plan[s]:
                assert c.plan[s]["pj_tiles"] == D.pj_tiles(d.mel, d.r, 256 if _reference_sized(c) else d.prenet[0]), c.name
    # (a) the tile counts, beyond the 27 of the shipped model
    tiles = {c.plan[s]["pj_tiles"] for n in D.PERSIST_ROWS for c in [by[n]] for s in c.shapes}
    assert tiles == {32, 37, 42, 57, 80, 81} and all(_reference_sized(by[n]) for n in D.PERSIST_ROWS)
    assert any(not _padded(by[n]) and by[n].mixed is False for n in D.PERSIST_ROWS)         # full-size weights, fp32
    assert {_dims(by[n]).att_type for n in D.PERSIST_ROWS} == {"SMA", "BMA", "LSA"}
    lsa = [by[n] for n in D.PERSIST_ROWS if _dims(by[n]).att_type == "LSA"]
    assert all(s[1] <= 128 and s[0] <= 32 and c.plan[s]["persist"] for c in lsa for s in c.shapes)
    assert any(c.lengths for c in map(by.get, D.PERSIST_ROWS)) and any(_dims(by[n]).gst for n in D.PERSIST_ROWS)
    assert {(_dims(by[n]).mel, _dims(by[n]).r) for n in D.PERSIST_ROWS} == {(80, 5), (128, 5), (112, 9), (128, 8), (80, 3), (80, 4)}
    # both M-tile counts of the one-group kernel, the group kernels, the bf16 kernel
    persisting = [(by[n], s) for n in D.PERSIST_ROWS for s in by[n].shapes if by[n].plan[s]["persist"]]
    assert {(s[0] + 15) // 16 for c, s in persisting if s[0] <= 32 and not c.mixed} == {1, 2}
    assert any(s[0] > 64 for c, s in persisting if not c.mixed) and any(c.plan[s]["persist_bf16"] for c, s in persisting)
    # refused the persistent launch: the launch path with every lean form, or with the bf16 mirrors
    refused = [(by[n], s) for n in D.PERSIST_ROWS for s in by[n].shapes if not by[n].plan[s]["persist"]]
    assert any(all(c.plan[s].get(k) == v for k, v in D._LEAN_LAUNCH.items()) for c, s in refused)
    assert any(c.plan[s].get("mirror") == 1 for c, s in refused)
    # (b) own sizes: a dimension above the reference's, never padded
    own = [c for c in D.CASES if c.name not in D.PERSIST_ROWS]
    ref = D.SHIPPED["prenet"] + (D.SHIPPED["att"],) + D.SHIPPED["rnn"]
    for c in own:
        d = _dims(c)
        bigger = any(s > r for s, r in zip(tuple(d.prenet) + (d.att,) + tuple(d.dec_rnn), ref))
        assert (bigger or d.mel > 128) and not _padded(c) and all(p["persist"] == 0 for p in c.plan.values()), c.name
    rnn = {tuple(_dims(c).dec_rnn): c for c in own}
    assert {(1536, 1536), (1024, 1536), (1536, 1024)} <= set(rnn)
    p = rnn[(1536, 1536)].plan
    assert {s[0] for s in p} == {5, 37} and all((q["lean_x0"], q["lean_x1"], q["lean_rec"], q["lean_proj"], q["fuse12"]) == (1, 0, 0, 0, 0) for q in p.values())
    (q,) = rnn[(1024, 1536)].plan.values()
    assert (q["lean_x0"], q["lean_x1"], q["lean_rec"], q["lean_proj"]) == (1, 1, 0, 0)
    (q,) = rnn[(1536, 1024)].plan.values()
    assert (q["lean_x0"], q["lean_x1"], q["lean_rec"], q["lean_proj"]) == (1, 0, 0, 1)
    # the k-block counts those predicates look at, from the sizes (gt_lstm_x_supported: 24 or 64; gt_proj_lean_supported: 72 beside 64)
    for sizes, c in rnn.items():
        d = _dims(c)
        if sizes not in ((1536, 1536), (1024, 1536), (1536, 1024)):
            continue
        nkb_x = ((d.prenet[1] + d.att) // 16, sizes[0] // 16)
        (q,) = set(tuple(sorted(v.items())) for v in c.plan.values())
        q = dict(q)
        assert (q["lean_x0"], q["lean_x1"]) == tuple(int(n in (24, 64)) for n in nkb_x)
        assert q["lean_proj"] == int((sizes[1] + d.att) // 16 == 72 and sizes[1] // 16 == 64)
        assert q["lean_rec"] == int(sizes[0] // 16 == 64 and sizes[1] // 16 == 64)
    assert any(tuple(_dims(c).prenet) == (512, 256) and all(q["fused"] == 0 for q in c.plan.values()) for c in own)
    assert any(_dims(c).att == 256 and max(_dims(c).prenet) <= 128 for c in own)
    assert any(_dims(c).att in (144, 192) for c in own)
    # the front end's Mel_Dim limit: 128 fused (and persistent), 144 not, the decoder the shipped one on both sides
    assert any(_dims(by[n]).mel == 128 and all(q.get("fused", 1) == 1 for q in by[n].plan.values()) for n in D.PERSIST_ROWS)
    m144 = by["mel144_shipped"]
    assert _dims(m144).mel == 144 and _reference_sized(m144) and not _padded(m144) and all(q["fused"] == 0 for q in m144.plan.values())
    assert [c.name for c in own if c.mixed] == ["rnn1536x1024"] and by["rnn1536x1024"].mixed == "also"
    assert [c.name for c in own if c.forced] == ["rnn1024x1536"]
    assert sum(_dims(c).gst for c in D.CASES) in (1, 2)
    # masked runs: a full row 0, a row shorter than the batch's; explicit lengths, one per row
    for name, shape in MASKED:
        tl = D.inputs(name, shape).lengths
        assert len(tl) == shape[0] and tl[0] == shape[1] and 1 <= tl.min() < shape[1]


def test_persistent_rows_sit_on_both_sides_of_each_grid_inequality():
    """gt_persist_decode_supported (csrc/persist_decode.hip), from each row's own numbers.  One-group kernel (fp32, B <= 32):
    32 chain + pj_tiles x MT projection + 64 helper workgroups <= 256; group kernels (fp32, 32 < B <= 128): B + 2 x pj_tiles <= 256;
    bf16 kernel (B <= 64): 2 x B + pj_tiles x MT <= 256.  MT = ceil(B / 16), pj_tiles = (ceil((Mel_Dim x r + 1) / 16) x 16 + 256) / 16."""
    sides = {}
    for n in D.PERSIST_ROWS:
        c = D.BY_NAME[n]
        for s in c.shapes:
            B, MT, pj, bf16 = D.grid_numbers(n, s)
            assert pj == c.plan[s]["pj_tiles"] and B <= (64 if bf16 else 128)
            ((what, lhs),) = D.grid_inequalities(B, MT, pj, bf16).items()
            print("%-18s %-14s %s: %d -> %s" % (n, s, what, lhs, "persistent" if lhs <= D.PD_NWG else "launch path"))
            assert c.plan[s]["persist"] == int(lhs <= D.PD_NWG), (n, s, what, lhs)
            assert c.plan[s]["persist_bf16"] == int(bf16 and lhs <= D.PD_NWG)
            sides.setdefault(what, []).append(lhs)
    assert set(sides) == {"32 + pj_tiles*MT + 64 <= 256", "B + 2*pj_tiles <= 256", "2B + pj_tiles*MT <= 256"}
    for what, lhs in sides.items():
        assert D.PD_NWG in lhs, (what, "no row fills the grid exactly", lhs)            # the last shape admitted: the plain role is gone
        assert any(v > D.PD_NWG for v in lhs), (what, "no row is refused", lhs)
        assert any(v < D.PD_NWG for v in lhs), (what, lhs)
    # the plain role disappears exactly at the boundary of the one-group kernel
    assert D.PD_NWG - D.PD_UTT - D.PD_HELP - 80 * 2 == 0


# ---------------------------------------------------------------------------------------------------- what the mutations would do
SENSITIVE = ("p80x5_bma_masked", (5, 23, 6))


def _mutated(name, shape, mutate):
    hp, w = D.model_of(name)
    w = {k: np.array(v) for k, v in w.items()}
    mutate(hp, w)
    return D.run_oracle(hp, w, D.inputs(name, shape), shape[2])


def test_feeding_back_the_wrong_frame_moves_a_row_with_r_5():
    """What ``last = (r - 2) x Mel_Dim`` would compute -- in the frame fed back (DecodeCall::frame) or in the columns proj_z composes
    with prenet 0: the oracle on a model whose projection emits frames r - 2 and r - 1 in each other's place, frames swapped back."""
    name, shape = SENSITIVE
    mel, r = 80, 5
    assert _dims(D.BY_NAME[name]).r == r >= 3

    def swap(hp, w):
        for k in ("decoder.projection.kernel", "decoder.projection.bias"):
            a, b = w[k][..., (r - 2) * mel:(r - 1) * mel].copy(), w[k][..., (r - 1) * mel:r * mel].copy()
            w[k][..., (r - 2) * mel:(r - 1) * mel], w[k][..., (r - 1) * mel:r * mel] = b, a

    got = _mutated(name, shape, swap)
    B, S = shape[0], shape[2]
    pre = got["pre_mel"].reshape(B, S, r, mel)[:, :, [0, 1, 2, 4, 3]].reshape(B, S * r, mel)
    ref = D.reference(name, shape).ref
    moved = {"pre_mel": D.err(pre, ref["pre_mel"]), "stop": D.err(got["stop"], ref["stop"]), "align": D.err(got["align"], ref["align"])}
    print(name, shape, "fed back frame r - 2 instead of r - 1: the float64 oracle moves by", moved)
    assert D.err(pre[:, :r], ref["pre_mel"][:, :r]) < 1e-12             # (step 0 sees the zero go frame either way)
    assert min(moved.values()) > 100 * D.TOL


def test_shifting_the_prenet0_columns_by_a_tile_moves_a_row_with_r_5():
    """What z_col0 off by one 16-column tile would compute: prenet-0 unit j receives the pre-activation of unit j + 16."""
    name, shape = SENSITIVE

    def shift(hp, w):
        for k in ("decoder.prenet0.kernel", "decoder.prenet0.bias"):
            w[k] = np.roll(w[k], -16, axis=-1)

    got = _mutated(name, shape, shift)
    moved = D.errs(got, D.reference(name, shape).ref)
    print(name, shape, "prenet-0 columns shifted by one tile: the float64 oracle moves by", moved)
    assert min(moved[k] for k in D.LOOP_OUTPUTS) > 100 * D.TOL


@pytest.mark.parametrize("name,shape", MASKED, ids=_id)
def test_masked_rows_are_real(name, shape):
    tl = D.inputs(name, shape).lengths
    full, masked = D.reference(name, shape).ref, D.reference(name, shape, True).ref
    assert D.err(full["align"][0], masked["align"][0]) < 1e-12
    live = np.arange(shape[1])[None, :] < tl[:, None]
    assert not masked["align"].transpose(0, 2, 1)[~live].any()
    moved = D.err(full["pre_mel"][1:], masked["pre_mel"][1:])
    print(name, shape, "masked against unmasked oracle, pre_mel of the short rows: max abs", moved)
    assert moved > 100 * D.TOL


@pytest.mark.parametrize("name,shape", FORCED, ids=_id)
def test_forced_rows_are_real(name, shape):
    free, forced = D.reference(name, shape).ref, D.reference(name, shape, forced=True).ref
    moved = D.err(free["pre_mel"], forced["pre_mel"])
    print(name, shape, "forced against free-running oracle: max abs", moved)
    assert forced["pre_mel"].shape == free["pre_mel"].shape and moved > 100 * D.TOL


# ---------------------------------------------------------------------------------------------------- the library without a device
@pytest.fixture(scope="module")
def lib():
    from gst_tacotron_amd import build, capi
    build.build()
    return capi.load_library()


def test_c_manifest_matches_python_manifest_on_every_row(lib):
    from gst_tacotron_amd import capi
    for c in D.CASES:
        hp = D.hp_case(**c.hp)
        ctx = capi.Context(hp, max_batch=2, max_tokens=8, max_ref_frames=D.TREF + 1)
        assert list(ctx.manifest().items()) == [(k, tuple(v)) for k, v in weights.manifest(hp).items()], c.name
        ctx.close()


@pytest.mark.parametrize("what,override,field", D.REFUSALS, ids=[r[0] for r in D.REFUSALS])
def test_create_refuses_by_name(lib, what, override, field):
    """gsttaco_create touches no HIP call before gsttaco_finalize_weights: the refusals hold with no device."""
    from gst_tacotron_amd import capi
    hp = D.refusal_hp(override)
    # (Step_Reduction 0 does not get as far as create through the Python surface: hparams.Dims divides by it and refuses it by name)
    with pytest.raises(ValueError if override.get("r") == 0 else capi.GstTacoError) as e:
        capi.Context(hp, max_batch=2, max_tokens=8, max_ref_frames=9).close()
    print(what, "->", e.value)
    assert field in str(e.value)


@pytest.mark.parametrize("r,max_step", [(0, 24), (5, 4)], ids=["Step_Reduction 0", "Max_Step < Step_Reduction"])
def test_create_itself_refuses_the_step_settings(lib, r, max_step):
    """The same two settings handed to gsttaco_create directly, past hparams.Dims."""
    import ctypes
    from gst_tacotron_amd import capi
    cfg = capi.make_config(D.refusal_hp({}), max_batch=2, max_tokens=8, max_ref_frames=9)
    cfg.step_reduction, cfg.max_step = r, max_step
    h = ctypes.c_void_p()
    assert lib.gsttaco_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    msg = lib.gsttaco_last_error(None).decode()
    print(msg)
    assert "Step_Reduction" in msg and "Max_Step" in msg


def test_the_tiny_decoder_of_the_refusals_is_accepted(lib):
    from gst_tacotron_amd import capi
    capi.Context(D.refusal_hp({}), max_batch=2, max_tokens=8, max_ref_frames=9).close()


def test_plan_reporter_is_declared_bound_and_needs_a_finalized_context(lib):
    import ctypes
    from gst_tacotron_amd import capi
    from gst_tacotron_amd.model import GST_Tacotron
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    assert re.search(r"\bint\s+gsttaco_decode_plan_fields\s*\(", header) and "gsttaco_decode_plan_fields" in capi.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+GSTTACO_ABI_VERSION\s+14\b", header) and capi.ABI_VERSION == 14          # (additive: no version step)
    ids = {n.lower(): int(v) for n, v in re.findall(r"GSTTACO_PLAN_([A-Z0-9_]+)\s*=\s*(\d+)", header)}
    assert ids.pop("count") == len(capi.PLAN_FIELDS)
    assert ids == {n: i for i, n in enumerate(capi.PLAN_FIELDS)}
    assert callable(GST_Tacotron.decode_plan_fields)
    # ONE copy of the logic: the reporter calls plan_decode, as gsttaco_decode_plan does
    src = open(os.path.join(ROOT, "gst_tacotron_amd", "csrc", "gsttaco.cpp")).read()
    body = src[src.index("int gsttaco_decode_plan_fields("):]
    body = body[:body.index("\n}\n")]
    assert "plan_decode(c, c->allow, B, Tv, false, forced != 0)" in body and "gt_" not in body
    ctx = capi.Context(D.refusal_hp({}), max_batch=2, max_tokens=8, max_ref_frames=9)
    out = (ctypes.c_int32 * len(capi.PLAN_FIELDS))()
    assert lib.gsttaco_decode_plan_fields(ctx.handle, 2, 8, 0, out) == -1           # (not finalized: as the *_variants reporters)
    ctx.close()
