"""CPU: the table of tests/hp_surface_cases.py is sound (no GPU involved: these are properties of the cases, of the two oracles, of the
manifests and of gsttaco_create, not of the kernels)."""
import numpy as np
import pytest

import hp_surface_cases as H
from gst_tacotron_amd import hparams, tf_checkpoint, weights
from oracle import oracle_np

NAMES = [c.name for c in H.CASES]
CALLS = [(c.name, s) for c in H.CASES for s in c.shapes]
MASKED = [(c.name, s) for c in H.CASES if c.lengths for s in c.lengths]
MIXED = [(c.name, s) for c in H.CASES if c.mixed for s in c.shapes]
ORACLE_BAR = 1e-9           # oracle/gen_golden.py's own bar between the two oracles


def _id(v):
    return v if isinstance(v, str) else "x".join(map(str, v))


def _dims(c):
    return hparams.Dims(H.model_of(c.name)[0])


def _torch(name):
    import torch
    from oracle.torch_ref import TorchReference
    hp, w = H.model_of(name)
    return torch, TorchReference(hp, w, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------- the two oracles agree
@pytest.mark.parametrize("name,shape", [(n, s) for n, s in CALLS if H.BY_NAME[n].module != "postnet"], ids=_id)
def test_oracles_agree_in_float64(name, shape):
    """oracle_np against torch_ref (torch's own conv1d / max_pool1d / fused LSTM cell).  (There is no stand-alone torch_ref postnet:
    the end-to-end cases cover it.)"""
    torch, tr = _torch(name)
    x = H.inputs(name, shape)
    with torch.no_grad():
        got = tr.encoder(x) if H.BY_NAME[name].module == "encoder" else tr.vocoder(torch.as_tensor(np.asarray(x, np.float64)))
    e = H.err(got.numpy(), H.reference(name, shape).ref)
    print(name, shape, "oracle_np against torch_ref, float64: max abs", e)
    assert e <= ORACLE_BAR


@pytest.mark.parametrize("name", list(H.E2E))
def test_end_to_end_oracles_agree_in_float64(name):
    torch, tr = _torch(name)
    c = H.e2e_case(name)
    ref, _ = H.e2e_reference(name)
    mel, stop, spec, align, inter = tr.inference_step(c.tokens, c.mels, c.mel_lengths, c.masks, c.noise, steps=c.steps, with_vocoder=True)
    got = dict(zip(H.E2E_OUTPUTS, (mel, stop, spec, align, inter["pre_mel"])))
    errs = {k: H.err(got[k].numpy(), ref[k]) for k in H.E2E_OUTPUTS}
    print(name, "oracle_np against torch_ref, float64:", errs)
    assert max(errs.values()) <= ORACLE_BAR


# ---------------------------------------------------------------------------------------------------- admission
@pytest.mark.parametrize("name,shape", CALLS + [(n + "/masked", s) for n, s in MASKED], ids=_id)
def test_cases_are_admitted_by_the_oracle_alone(name, shape):
    """8 x the float32 floor is at most TOL: the GPU bound max(TOL, 8 x floor) is then TOL for every row.  A row that fails here is
    replaced, never widened."""
    masked = name.endswith("/masked")
    name = name.split("/")[0]
    r = H.reference(name, shape, masked)
    print(name, shape, "masked" if masked else "", "float32 oracle against float64: max abs %.3g scale %.3g" % (r.floor, r.scale))
    assert np.isfinite(r.ref).all() and r.scale > 0.01
    assert H.FLOOR_FACTOR * r.floor <= H.TOL
    assert H.tolerance(r.floor) == H.TOL


@pytest.mark.parametrize("name", list(H.E2E))
def test_end_to_end_cases_are_admitted(name):
    ref, floor = H.e2e_reference(name)
    print(name, "float32 oracle against float64:", floor)
    for k in H.E2E_OUTPUTS:
        assert np.isfinite(ref[k]).all() and H.FLOOR_FACTOR * floor[k] <= H.TOL, (k, floor[k])


# ---------------------------------------------------------------------------------------------------- coverage of the table itself
def test_table_covers_what_it_claims():
    enc = [c for c in H.CASES if c.module == "encoder"]
    post = [c for c in H.CASES if c.module == "postnet"]
    voc = [c for c in H.CASES if c.module == "vocoder"]
    rnn = {_dims(c).enc_rnn for c in enc} | {_dims(c).voc_rnn for c in voc}
    assert rnn >= {48, 128, 256}
    # an odd first-segment k-block count of the general skinny BiLSTM: C = the last conv's filters (encoder), Highwaynet.Size (vocoder)
    assert any((_dims(c).enc_filters[-1] // 16) % 2 == 1 and _dims(c).enc_rnn != 256 for c in enc)
    kernels = {k for c in enc for k in _dims(c).enc_kernels}
    assert 1 in kernels and any(k % 2 == 0 for k in kernels) and any(k > 5 for k in kernels)
    assert {len(_dims(c).enc_filters) for c in enc} >= {1, 8}
    assert {len(_dims(c).post_filters) for c in post} >= {2, 8}              # (the postnet cannot have fewer than 2: post_tanh = 0)
    assert any(_dims(c).post_tanh == 0 for c in post)
    assert any(_dims(c).emb % 16 for c in enc)
    assert any(_dims(c).emb > max(_dims(c).enc_filters) for c in enc)
    assert any(f % 16 for c in post for f in _dims(c).post_filters)
    combos = set()
    for c in voc:
        m = weights.manifest(H.model_of(c.name)[0])
        combos.add(("vocoder.proj_dense.kernel" in m, "vocoder.highway_in.kernel" in m))
    assert combos == {(False, False), (True, False), (False, True), (True, True)}
    assert 0 in {_dims(c).highway_count for c in voc}
    assert 32 in {_dims(c).bank_count for c in voc}
    assert any(len(_dims(c).voc_proj_filters) == 1 for c in voc)
    # the two gates, by the host's own arithmetic (csrc/gsttaco.cpp encoder_rows_path; csrc/gemm_conv.hip gt_conv_gemm_variant)
    d = _dims(H.BY_NAME["enc_wino_odd"])
    (B, Tv), = H.BY_NAME["enc_wino_odd"].shapes
    wgs = [(B * ((Tv + 1) // 2) + 63) // 64 * ((f + 127) // 128) for f in d.enc_filters]
    assert wgs == [105, 210, 105] and min(wgs) >= 100 and d.emb % 4 == 0 and d.emb % 16
    (B, Tf), = H.BY_NAME["post_wino_small"].shapes
    assert (B * ((Tf + 3) // 4) + 63) // 64 == 240
    # every masked run has a full row 0 and a row shorter than the batch; explicit lengths, one per row
    for name, shape in MASKED:
        tl = H.lengths_of(name, shape)
        assert len(tl) == shape[0] and tl[0] == shape[1] and tl.min() >= 1 and tl.min() < shape[1]
    assert {n for n, _ in MASKED} == {"enc_k3_k1_k7_rnn48", "enc_one_even_rnn128", "enc_wino_odd"}
    assert {n for n, _ in MIXED} == {"enc_k3_k1_k7_rnn48", "enc_rnn256_c32", "post_mixed_kernels", "voc_no_dense", "voc_no_highway"}
    # the end-to-end cases are made of rows of the table
    for name, parts in (("e2e_odd_gst", ("enc_k3_k1_k7_rnn48", "post_mixed_kernels", "voc_no_dense")),
                        ("e2e_rnn256_nogst", ("enc_rnn256_c32", "voc_no_highway"))):
        for p in parts:
            assert H.BY_NAME[p].hp.items() <= H.E2E[name]["hp"].items(), (name, p)
    d = hparams.Dims(H.model_of("e2e_odd_gst")[0])
    assert d.mem == 112 and d.mem % 32 and d.r == 3 and hparams.Dims(H.model_of("e2e_rnn256_nogst")[0]).r == 1


@pytest.mark.parametrize("name,shape", MASKED, ids=_id)
def test_masked_cases_are_real(name, shape):
    """The masked oracle differs from the unmasked one by more than 100 x TOL on a row that is NOT padding, and row 0 is whole."""
    tl = H.lengths_of(name, shape)
    full, masked = H.reference(name, shape).ref, H.reference(name, shape, True).ref
    assert tl[0] == shape[1] and H.err(full[0], masked[0]) == 0.0
    live = np.arange(shape[1])[None, :] < tl[:, None]
    moved = np.abs(full - masked).max(-1)
    print(name, shape, "masked against unmasked oracle on the live positions: max abs", float(moved[live].max()))
    assert moved[live].max() > 100 * H.TOL
    assert not masked[~live].any()


@pytest.mark.parametrize("name,shape", MIXED, ids=_id)
def test_mixed_cases_are_real(name, shape):
    """The float64 and float32 evaluations of the bf16 emulation agree within drift / 16: no flipped rounding in the reference itself."""
    m = H.mixed_reference(name, shape)
    print(name, shape, "emulated-mixed against fp32 oracle (drift) %.3g, float64 against float32 emulation %.3g, GPU bound %.3g"
          % (m.drift, m.spread, H.mixed_tolerance(m.drift)))
    assert np.isfinite(m.ref).all() and H.mixed_tolerance(m.drift) > H.TOL       # (the bound leaves room for fp32 noise)
    assert m.spread <= m.drift / 16


# ---------------------------------------------------------------------------------------------------- what the mutations would do
@pytest.mark.parametrize("name", ["voc_no_dense", "voc_no_highway", "voc_highway_in_only"])
def test_dropping_the_epilogue_residual_moves_the_vocoder(name, monkeypatch):
    """What deleting ``a.res = mel_in`` in enqueue_vocoder would compute: the oracle without the residual, far beyond TOL."""
    c = H.BY_NAME[name]
    hp, w = H.model_of(name)
    assert "vocoder.proj_dense.kernel" not in w
    x = np.asarray(H.inputs(name, c.shapes[0]), np.float64)
    ref = H.reference(name, c.shapes[0]).ref                                # (before the oracle is patched)
    n = len(hp["Vocoder_Taco1"]["CBHG"]["Conv1D"]["Filters"])
    bn = oracle_np.batch_norm
    # (the residual is `y + x` behind the last projection's BN: take x off again right there)
    monkeypatch.setattr(oracle_np, "batch_norm", lambda y, ww, p: bn(y, ww, p) - (x if p == "vocoder.proj%d.bn" % (n - 1) else 0.0))
    moved = H.err(oracle_np.vocoder_taco1(hp, oracle_np.cast_weights(w, np.float64), x, np.float64), ref)
    print(name, "without the residual the spectrogram moves by", moved)
    assert moved > 100 * H.TOL


def test_symmetric_padding_moves_the_even_kernel_case(monkeypatch):
    """What pad_before = (k - 1) / 2 + (k % 2 == 0) in place of same_pad_before would compute on enc_one_even_rnn128."""
    name, shape = "enc_one_even_rnn128", (17, 3)
    same_pad = oracle_np.same_pad
    ref = H.reference(name, shape).ref                                      # (before the oracle is patched)

    def shifted(n_in, k, s):
        out, before, after = same_pad(n_in, k, s)
        return (out, before + 1, after - 1) if k % 2 == 0 else (out, before, after)

    monkeypatch.setattr(oracle_np, "same_pad", shifted)
    moved = H.err(H.oracle(name, shape), ref)
    print(name, "with one more frame of padding in front the encoding moves by", moved)
    assert moved > 100 * H.TOL


# ---------------------------------------------------------------------------------------------------- manifests and refusals
@pytest.fixture(scope="module")
def lib():
    from gst_tacotron_amd import build, capi
    build.build()
    return capi.load_library()


def _all_hps():
    return [(n, H.model_of(n)[0]) for n in NAMES + list(H.E2E)]


def test_c_manifest_matches_python_manifest_on_every_hp(lib):
    from gst_tacotron_amd import capi
    for name, hp in _all_hps():
        ctx = capi.Context(hp, max_batch=2, max_tokens=8, max_ref_frames=9)
        assert list(ctx.manifest().items()) == [(k, tuple(v)) for k, v in weights.manifest(hp).items()], name
        ctx.close()


def test_reference_paths_name_every_tensor_once():
    for name, hp in _all_hps():
        paths, man = tf_checkpoint.reference_paths(hp), weights.manifest(hp)
        assert set(paths) == set(man), (name, set(paths) ^ set(man))
        assert len(set(paths.values())) == len(paths), name                 # (no two tensors read the same checkpoint object)


@pytest.mark.parametrize("what,override,field", H.REFUSALS, ids=[r[0] for r in H.REFUSALS])
def test_create_refuses_by_name(lib, what, override, field):
    from gst_tacotron_amd import capi
    hp = H.hp_case(**override)
    with pytest.raises((capi.GstTacoError, ValueError)) as e:
        capi.Context(hp, max_batch=2, max_tokens=8, max_ref_frames=9).close()
    print(what, "->", e.value)
    assert field in str(e.value)


def test_dims_refuses_strides_and_pool_sizes():
    hp = H.hp_case()
    hp["Tacotron2"]["Encoder"]["Conv"]["Strides"] = [1, 2, 1]
    with pytest.raises(ValueError, match="strides"):
        hparams.Dims(hp)
    hp = H.hp_case()
    hp["Vocoder_Taco1"]["CBHG"]["Pool"]["Pool_Size"] = 3
    with pytest.raises(ValueError, match="Pool"):
        hparams.Dims(hp)
