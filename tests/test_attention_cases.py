"""CPU: the table of tests/attention_cases.py is sound (no GPU involved: these are properties of the rows, of the two oracles and of
gsttaco_create, not of the kernels)."""
import re

import numpy as np
import pytest

import attention_cases as A
import decoder_surface_cases as D
from gst_tacotron_amd import hparams

ROWS = A.CASES + [A.BOUNDARY]
RUNS = [(c.name + ("/" + mode if mode else ""), s) for c in ROWS for s, mode in A.runs_of(c)]
WRONG = [(c.name + ("/" + mode if mode else ""), s, w) for c in A.CASES for s, mode in A.runs_of(c) if mode != "forced" for w in c.wrong]


def _id(v):
    return v if isinstance(v, str) else "x".join(map(str, v))


# ---------------------------------------------------------------------------------------------------- admission
@pytest.mark.parametrize("name,shape", RUNS, ids=_id)
def test_rows_are_admitted_by_the_oracle_alone(name, shape):
    """8 x the float32 floor is at most TOL on every output: the GPU bound is TOL on every row.  A row that fails here is replaced,
    never widened."""
    name, _, mode = name.partition("/")
    r = A.reference(name, shape, mode == "masked", mode == "forced")
    print(name, shape, mode, "float32 oracle against float64:", {k: "%.3g" % v for k, v in r.floor.items()},
          "scale", {k: "%.3g" % v for k, v in r.scale.items()})
    B, Tv, steps = shape
    assert r.ref["mel"].shape == r.ref["pre_mel"].shape == (B, steps * A.MODEL["r"], A.MODEL["mel"])
    assert r.ref["stop"].shape == (B, steps) and r.ref["align"].shape == (B, steps, Tv)
    for k in D.OUTPUTS:
        assert np.isfinite(r.ref[k]).all() and r.scale[k] > 0.01, k
        assert D.FLOOR_FACTOR * r.floor[k] <= A.TOL, (k, r.floor[k])


@pytest.mark.parametrize("name,shape,which", WRONG, ids=_id)
def test_rows_tell_their_setting_from_the_mistake_they_exist_for(name, shape, which):
    """The float64 oracle with the setting wrong -- the default noise scale, Cumulate_Weights true, an even kernel's zeros the other way
    round -- lies at least 4 x TOL from the reference in ``align``: a kernel (or host predicate) making that mistake cannot pass the
    GPU test's TOL.  This is the CPU mutation of the code sites the table's docstring lists."""
    name, _, mode = name.partition("/")
    r = A.reference(name, shape, mode == "masked")
    moved = D.errs(A.wrong_setting(name, shape, which, mode == "masked"), r.ref)
    print("%-22s %-12s %-7s %-9s the float64 oracle moves by %s; float32 floor of align %.2g" % (
        name, shape, mode, which, " ".join("%s %.3g" % kv for kv in moved.items()), r.floor["align"]))
    assert moved["align"] >= A.DISTINCT, (which, moved)
    assert moved["align"] >= 100 * r.floor["align"]


@pytest.mark.parametrize("name", [c.name for c in ROWS])
def test_oracles_agree_in_float64(name):
    """oracle_np against oracle/torch_ref.py (torch's own conv1d with its own padding arithmetic, its own statement of Cumulate_Weights,
    Smoothing and Sigmoid_Noise) on every row's unmasked calls."""
    import torch
    from oracle.torch_ref import TorchReference
    hp, w = A.model_of(name)
    tr = TorchReference(hp, {k: np.array(v) for k, v in w.items()}, dtype=torch.float64)      # (writable copies: torch wants them)
    for shape in A.BY_NAME[name].shapes:
        x = A.inputs(name, shape)
        with torch.no_grad():
            memory = tr.encoder(np.array(x.tokens))
            masks = [tuple(torch.as_tensor(m) for m in ms) for ms in D.split_masks(hp, x.masks, shape[0])]
            pre, mel, stop, align = tr.decoder(memory, masks, torch.as_tensor(np.asarray(x.noise, np.float64)), shape[2])
        got = {"mel": mel.numpy(), "stop": stop.numpy(), "align": align.numpy(), "pre_mel": pre.numpy()}
        e = D.errs(got, A.reference(name, shape).ref)
        print(name, shape, "oracle_np against torch_ref, float64:", e)
        assert max(e.values()) <= A.ORACLE_BAR <= A.TOL


def test_wrong_padding_is_what_it_says():
    """The "lpad" mistake on a bare convolution: k // 2 zeros in front is the right result one position late -- and nothing else."""
    from oracle import oracle_np
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 11, 1))
    for k in (2, 4, 8, 30):
        kern = rng.standard_normal((k, 1, 3))
        right = oracle_np.conv1d_same(x, kern)
        assert oracle_np.same_pad(11, k, 1)[1:] == ((k - 1) // 2, k // 2)
        with A._wrong_padding():
            assert oracle_np.same_pad(11, k, 1)[1:] == (k // 2, (k - 1) // 2)
            wrong = oracle_np.conv1d_same(x, kern)
        assert np.abs(wrong[:, 1:] - right[:, :-1]).max() < 1e-12 and np.abs(wrong - right).max() > 0.1
    for k in (1, 5, 81):                            # odd kernels are symmetric: untouched
        with A._wrong_padding():
            assert oracle_np.same_pad(11, k, 1) == A._SAME_PAD(11, k, 1)
    assert oracle_np.same_pad is A._SAME_PAD


# ---------------------------------------------------------------------------------------------------- coverage of the table itself
def test_table_covers_the_settings_it_claims():
    by = A.BY_NAME
    dims = {c.name: hparams.Dims(A.hp_of(c.att)) for c in ROWS}
    for c in ROWS:
        d = dims[c.name]
        assert (d.mel, d.r, tuple(d.prenet), d.att, tuple(d.dec_rnn), d.gst) == (16, 2, (128, 128), 64, (512, 512), False), c.name
        assert set(c.plan) <= set(A.PATHS) and "four" in c.plan and all(4 <= s[2] <= 8 for s in c.shapes)
        for path in c.plan:
            for s in c.shapes:
                p = A.plan_of(c.name, path, s)
                assert p["dec_padded"] == 1 and p["fused"] == int(path != "four") and (path == "default" or p["persist"] == 0), (c.name, path)
        for s, tl in (c.lengths or {}).items():
            assert s in c.shapes and len(tl) == s[0] and tl[0] == s[1] and 1 <= min(tl) < s[1]
    # (a) the noise scale: 0 under SMA, a value that is neither 0, 1 nor 2, noise under BMA; each at both shapes, on all three paths,
    # persistent on the default path (5 rows: the one-group kernel; 37: the group kernels)
    noise = [c for c in A.CASES if c.att["Type"] != "LSA"]
    assert {(c.att["Type"], dims[c.name].sigmoid_noise) for c in noise} == {("SMA", 0.0), ("SMA", 0.5), ("BMA", 1.0)}
    for c in noise:
        assert c.shapes == [A.S5, A.S37] and set(c.plan) == set(A.PATHS) and "throughput" in c.extra and c.wrong == ("noise",)
        assert all(A.plan_of(c.name, "default", s)["persist"] == 1 for s in c.shapes)
        assert A.plan_of(c.name, "fused", A.S5)["lean_front"] == 1
    assert A.S5[0] <= 32 < A.S37[0] <= 128
    assert [c.name for c in noise if "noise_optional" in c.extra] == ["sma_noise0"]
    bma = by["bma_noise1"]
    assert set(bma.lengths) == set(bma.shapes) and all({1, 2} <= set(tl) for tl in bma.lengths.values())
    # (b) Cumulate_Weights false: softmax and smoothing, masked and not; two passes of the 128-row tile off the persistent chain; forced
    last = [c for c in A.CASES if c.att["Type"] == "LSA" and not dims[c.name].lsa_cumulate]
    assert all("cumulate" in c.wrong for c in last)
    assert {dims[c.name].lsa_smoothing for c in last if (dims[c.name].loc_filters, dims[c.name].loc_kernel) == (20, 9)} == {False, True}
    assert all(c.lengths for c in last if (dims[c.name].loc_filters, dims[c.name].loc_kernel) == (20, 9))
    long_ = by["lsa32x31_last_long"]
    assert long_.shapes == [A.LONG] and A.LONG[1] > 128 and long_.lengths[A.LONG] == (140, 60, 101)
    assert all(A.plan_of(long_.name, p, A.LONG)["persist"] == 0 for p in A.PATHS)
    assert [c.name for c in A.CASES if "forced" in c.extra] == ["lsa20x9_last"]
    # (c) taps and filters: six counts off the granules, every even one against the wrong padding, Cumulate_Weights false on half
    taps = {(dims[c.name].loc_filters, dims[c.name].loc_kernel): c for c in A.CASES if c.att["Type"] == "LSA" and c.shapes == [A.S5]
            and (dims[c.name].loc_filters, dims[c.name].loc_kernel) != (20, 9)}
    assert set(taps) == {(20, 8), (17, 4), (1, 2), (32, 30), (8, 1), (12, 81)}
    for (f, k), c in taps.items():
        assert ("lpad" in c.wrong) == (k % 2 == 0) and ("cumulate" in c.wrong) == (not dims[c.name].lsa_cumulate) and c.wrong
        assert A.plan_of(c.name, "default", A.S5)["persist"] == 1 and set(c.plan) == set(A.PATHS)
    assert sum(not dims[c.name].lsa_cumulate for c in taps.values()) == 3
    over = taps[(12, 81)]
    assert (81 - 1) // 2 + 81 // 2 > A.S5[1] and {1, 2} <= set(over.lengths[A.S5])      # every window overhangs both ends
    assert any(f % 16 == 1 and f > 16 for f, _ in taps) and any(f == 1 for f, _ in taps) and any(k % 4 for _, k in taps)


def test_sigmoid_noise_of_an_lsa_model_is_zero_whatever_the_key_says():
    for sn in (0.0, 0.5, 2.0):
        att = dict(A.BY_NAME["lsa20x9_last"].att, Sigmoid_Noise=sn)
        assert hparams.Dims(A.hp_of(att)).sigmoid_noise == 0.0
    assert hparams.Dims(A.hp_of({"Type": "SMA", "Size": 64})).sigmoid_noise == 2.0
    assert hparams.Dims(A.hp_of({"Type": "BMA", "Size": 64})).sigmoid_noise == 0.0
    assert hparams.Dims(A.hp_of({"Type": "BMA", "Size": 64, "Sigmoid_Noise": 1.0})).sigmoid_noise == 1.0
    assert hparams.Dims(A.hp_of({"Type": "SMA", "Size": 64, "Sigmoid_Noise": 0.0})).sigmoid_noise == 0.0


# ---------------------------------------------------------------------------------------------------- what create admits
@pytest.fixture(scope="module")
def lib():
    from gst_tacotron_amd import build, capi
    build.build()
    return capi.load_library()


def _bytes(att, max_tokens, att_run=A.ATT_RUN):
    conv = att.get("Conv", {})
    lsa = att["Type"] == "LSA"
    return A.attn_lds_bytes(max_tokens, att_run, conv["Filters"] if lsa else 0, conv["Kernel_Size"] if lsa else 0)


def test_the_boundary_row_sits_just_inside_the_limit():
    """By the byte function alone: 128 filters x 103 taps at 37 tokens and Attention.Size 128 (as run) fits, one more tap does not; the
    largest pair inside the 1..128 x 1..255 bounds, 128 x 255, needs about 242 KB; SMA / BMA fit up to 7 701 tokens."""
    assert _bytes(A.BOUNDARY.att, 37) == 163812 <= A.LDS_LIMIT == 163840 < _bytes(A._lsa(128, 104), 37) == 164324
    assert _bytes(A._lsa(128, 255), 37) == 241636
    sma = {"Type": "SMA", "Size": 64}
    assert _bytes(sma, A.MAX_TOKENS_LIMIT) <= A.LDS_LIMIT < _bytes(sma, A.MAX_TOKENS_LIMIT + 1)
    assert A.BOUNDARY_SHAPE[1] == 37 and set(A.BOUNDARY.plan) == {"four"}
    # every other row of the GPU table is well inside at its own capacity (max_tokens = Tv): at most 32 x 31 at 140 tokens, 119 280 bytes
    for c in A.CASES:
        assert all(_bytes(c.att, s[1]) <= 119280 for s in c.shapes), c.name
    for what, att, max_tokens, _, over in A.ATT_REFUSALS:
        conv = att.get("Conv", {})
        in_bounds = att["Type"] != "LSA" or (1 <= conv["Filters"] <= 128 and 1 <= conv["Kernel_Size"] <= 255)
        assert over == in_bounds and (not over or _bytes(att, max_tokens) > A.LDS_LIMIT), what
    for what, att, max_tokens in A.ATT_ADMITTED:
        assert _bytes(att, max_tokens) <= A.LDS_LIMIT, what


@pytest.mark.parametrize("what,att,max_tokens,field,over", A.ATT_REFUSALS, ids=[r[0] for r in A.ATT_REFUSALS])
def test_create_refuses_by_name(lib, what, att, max_tokens, field, over):
    """gsttaco_create touches no HIP call before gsttaco_finalize_weights: the refusals hold with no device, and nothing is launched to
    find the limit.  Over the limit the message carries the byte count: it is the restated function's."""
    from gst_tacotron_amd import capi
    with pytest.raises(capi.GstTacoError) as e:
        capi.Context(A.hp_of(att), max_batch=2, max_tokens=max_tokens, max_ref_frames=9).close()
    print(what, "->", e.value)
    assert field in str(e.value)
    if over:
        m = re.search(r"needs (\d+) bytes of LDS .* more than the (\d+) a", str(e.value))
        assert m and int(m.group(1)) == _bytes(att, max_tokens) and int(m.group(2)) == A.LDS_LIMIT


@pytest.mark.parametrize("what,att,max_tokens", A.ATT_ADMITTED, ids=[r[0] for r in A.ATT_ADMITTED])
def test_create_admits_what_fits(lib, what, att, max_tokens):
    from gst_tacotron_amd import capi
    capi.Context(A.hp_of(att), max_batch=2, max_tokens=max_tokens, max_ref_frames=9).close()


def test_the_limit_goes_by_the_attention_size_as_run(lib, monkeypatch):
    """Attention.Size 64 runs at the reference's 128 where pad_decoder embeds the model, at 64 under GSTTACO_PAD_DECODER=0: 128 x 104
    then fits (121 060 bytes), 128 x 255 (198 372) still does not."""
    from gst_tacotron_amd import capi
    monkeypatch.setenv("GSTTACO_PAD_DECODER", "0")
    assert _bytes(A._lsa(128, 104), 37, 64) == 121060 and _bytes(A._lsa(128, 255), 37, 64) == 198372
    capi.Context(A.hp_of(A._lsa(128, 104)), max_batch=2, max_tokens=37, max_ref_frames=9).close()
    with pytest.raises(capi.GstTacoError) as e:
        capi.Context(A.hp_of(A._lsa(128, 255)), max_batch=2, max_tokens=37, max_ref_frames=9).close()
    assert "Attention.Conv" in str(e.value) and "198372" in str(e.value)
    # a decoder at the reference's own sizes is not padded: Attention.Size 128 as given
    monkeypatch.delenv("GSTTACO_PAD_DECODER")
    hp = D.hp_case(mel=16, r=2, att_type="LSA")
    hp["Tacotron2"]["Decoder"]["Attention"] = dict(A._lsa(128, 104), Size=128)
    with pytest.raises(capi.GstTacoError) as e:
        capi.Context(hp, max_batch=2, max_tokens=37, max_ref_frames=9).close()
    assert "164324" in str(e.value)
