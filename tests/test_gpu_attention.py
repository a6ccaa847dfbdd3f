"""GPU: the attention's settings off their defaults (tests/attention_cases.py: Sigmoid_Noise, Cumulate_Weights, Smoothing, even tap counts,
filter counts off the MFMA granules, the row just inside gsttaco_create's LDS limit) against the float64 oracle, every row on each path its
plan names -- the four-kernel front end, the fused launch path, the persistent launch -- one context alive at a time.  Every run asserts
the plan fields the row states for the path (gsttaco_decode_plan_fields) and what decode_counters() says about the persistent launch: a
row that lands on another path fails.  fp32; the bound is TOL on mel (pre- and post-postnet), stop and alignment -- every row is admitted
at 8 x the oracle's float32 floor <= TOL, and tells its setting from the mistake it exists for by at least 4 x TOL, by
tests/test_attention_cases.py."""
import gc

import numpy as np
import pytest

import attention_cases as A
import decoder_surface_cases as D
from test_gpu_decoder_surface import KNOBS, _assert_bitwise, _assert_counters, _check, _plan
from test_gpu_parity import _model, _sole_context

pytestmark = pytest.mark.gpu

CALLS = [(c.name, s) for c in A.CASES for s in c.shapes]
THROUGHPUT = [(c.name, s) for c in A.CASES if "throughput" in c.extra for s in c.shapes]
FORCED = [(c.name, c.shapes[0]) for c in A.CASES if "forced" in c.extra]


def _id(v):
    return v if isinstance(v, str) else "x".join(map(str, v))


def _context(monkeypatch, name, shape, path):
    """A context of the row's model on ``path`` (the library reads its knobs once, at create)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in A.PATHS[path].items():
        monkeypatch.setenv(k, v)
    _sole_context()
    hp, w = A.model_of(name)
    return _model(hp, w, shape[0], shape[1], 2)


def _run(m, name, shape, masked=False, forced=False, seed=None, noise=True):
    """One Inference_Step of the row's inputs with injected randomness (``noise`` False: keep masks only; ``seed``: throughput mode
    instead) -> {output: array}."""
    import torch
    x = A.inputs(name, shape)
    kw = dict(seed=seed) if seed is not None else dict(prenet_masks=x.masks, attn_noise=x.noise if noise else None)
    if forced:
        kw["teacher_mels"] = A.teacher(shape)
    else:
        kw["steps"] = shape[2]
    out = m.Inference_Step(x.tokens, x.lengths if masked else None, None, None, None, return_pre_mel=True, masked=masked, **kw)
    m.synchronize()
    torch.cuda.synchronize()
    mel, stop, _, align, pre = out
    assert m.handoff_error() == 0
    return {k: t.cpu().numpy() for k, t in (("mel", mel), ("stop", stop), ("align", align), ("pre_mel", pre))}


def _check_alignment(what, name, shape, got, masked):
    """Zero beyond a masked length, exactly; an LSA alignment (softmax, or sigmoid / sum) sums to 1 over the positions that exist."""
    tl = A.inputs(name, shape).lengths if masked else None
    if tl is not None:
        for b, n in enumerate(tl):
            assert not got["align"][b][:, n:].any(), (what, b, n)
    if A.BY_NAME[name].att["Type"] == "LSA":
        s = got["align"].sum(-1, dtype=np.float64)
        assert np.abs(s - 1.0).max() <= 1e-5, (what, "alignment rows sum to", s.min(), s.max())


def _row_on_path(monkeypatch, name, shape, path):
    c = A.BY_NAME[name]
    want = A.plan_of(name, path, shape)
    masked = bool(c.lengths and shape in c.lengths)
    what = "%s %s %s" % (name, shape, path)
    m = _context(monkeypatch, name, shape, path)
    _plan(m, name, shape, want, path)
    got = _run(m, name, shape)
    calls = 1
    _check(what, got, A.reference(name, shape).ref)
    _check_alignment(what, name, shape, got, False)
    if masked:
        gm = _run(m, name, shape, masked=True)
        calls += 1
        _check(what + " masked", gm, A.reference(name, shape, True).ref)
        _check_alignment(what + " masked", name, shape, gm, True)
    if "noise_optional" in c.extra:
        # Sigmoid_Noise 0.0: the tensor is neither needed nor read -- the same plan, the same launches, the same bits
        assert hparams_noise(name) == 0.0
        bare = _run(m, name, shape, noise=False)
        calls += 1
        _plan(m, name, shape, want, path + ", no noise tensor")
        _check(what + " without a noise tensor", bare, A.reference(name, shape).ref)
        _assert_bitwise(got, bare, what + ": with against without a noise tensor")
    _assert_counters(m, bool(want["persist"]), name, shape, calls)
    del m
    gc.collect()


def hparams_noise(name):
    from gst_tacotron_amd import hparams
    return hparams.Dims(A.model_of(name)[0]).sigmoid_noise


@pytest.mark.parametrize("path", list(A.PATHS))
@pytest.mark.parametrize("name,shape", CALLS, ids=_id)
def test_rows_match_the_oracle_on_every_path(monkeypatch, name, shape, path):
    assert set(A.BY_NAME[name].plan) == set(A.PATHS)
    _row_on_path(monkeypatch, name, shape, path)


@pytest.mark.parametrize("name,shape", THROUGHPUT, ids=_id)
def test_device_noise_is_unscaled_and_the_same_on_every_path(monkeypatch, name, shape):
    """Throughput mode (seed=, nothing injected): the keep decisions and the noise come from the seed on the device.  The tensors the
    decode used are read back (gsttaco_debug_randomness): the noise is N(0, 1) as drawn -- the row's scale is the kernels' business -- and
    the same on the three paths; fed to the oracle at the row's scale they give the GPU's outputs.  With Sigmoid_Noise 0.0 no noise is
    drawn and none is looked at: the oracle gets zeros, which it ignores as well."""
    B, Tv, steps = shape
    scale = hparams_noise(name)
    n = steps * B * Tv
    runs = {}
    for path in A.PATHS:
        m = _context(monkeypatch, name, shape, path)
        want = A.plan_of(name, path, shape)
        _plan(m, name, shape, {k: want[k] for k in ("fused", "persist", "dec_padded")}, path + ", throughput mode")
        got = _run(m, name, shape, seed=4242)
        masks, noise = m.debug_randomness(steps, B, Tv)
        _assert_counters(m, bool(want["persist"]), name, shape)
        runs[path] = (got, masks, noise)
        del m
        gc.collect()
    _, masks, noise = runs["four"]
    assert set(np.unique(masks)) <= {0.0, 1.0} and abs(masks.mean() - 0.5) < 4 * 0.5 / np.sqrt(masks.size)
    for path in ("fused", "default"):
        assert np.array_equal(masks, runs[path][1]), path
    if scale > 0.0:
        # 4 sigma of the sample mean and of the sample deviation of n standard normals: a tensor scaled by 0.5 (or 2) is far outside
        print("%s %s read-back noise: mean %.4f std %.4f over %d" % (name, shape, noise.mean(), noise.std(), n))
        assert np.isfinite(noise).all() and abs(noise.mean()) < 4 / np.sqrt(n) and abs(noise.std() - 1.0) < 4 / np.sqrt(2 * n)
        for path in ("fused", "default"):
            assert np.array_equal(noise, runs[path][2]), path
    else:
        noise = np.zeros((steps, B, Tv), np.float32)
    x = A.inputs(name, shape)._replace(masks=masks.reshape(steps, -1), noise=noise)
    ref = A.oracle(name, shape, x=x)
    for path, (got, _, _) in runs.items():
        _check("%s %s %s throughput mode" % (name, shape, path), got, ref)
    assert D.err(ref["align"], A.reference(name, shape).ref["align"]) > 100 * A.TOL          # (not the injected run over again)


@pytest.mark.parametrize("path", ["four", "fused"])
@pytest.mark.parametrize("name,shape", FORCED, ids=_id)
def test_last_step_state_teacher_forced(monkeypatch, name, shape, path):
    """forced_cases.forced_decoder follows Cumulate_Weights; a forced decode launches per step (the default path's plan is then the
    fused launch path's)."""
    want = dict(A.plan_of(name, path, shape), persist=0)
    m = _context(monkeypatch, name, shape, path)
    _plan(m, name, shape, want, path + ", forced", forced=True)
    got = _run(m, name, shape, forced=True)
    _assert_counters(m, False, name, shape)
    del m
    gc.collect()
    _check("%s %s %s forced" % (name, shape, path), got, A.reference(name, shape, forced=True).ref)
    _check_alignment("forced", name, shape, got, False)


def test_the_row_just_inside_the_create_limit_runs_on_the_four_kernel_path(monkeypatch):
    """128 filters x 103 taps at 37 tokens: 163 812 of the attention step's 163 840 bytes of LDS (tests/test_attention_cases.py has the
    arithmetic, and what create refuses beyond it)."""
    name, shape = A.BOUNDARY.name, A.BOUNDARY_SHAPE
    assert A.attn_lds_bytes(shape[1], A.ATT_RUN, 128, 103) == 163812 <= A.LDS_LIMIT
    _row_on_path(monkeypatch, name, shape, "four")
