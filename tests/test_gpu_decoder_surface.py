"""GPU: the decode loop off the shipped decoder sizes and Step_Reduction (tests/decoder_surface_cases.py) against the float64 oracle,
each call on a context of its own (max_batch = B, max_tokens = Tv; one live context at a time: the persistent forms need the process's
only one).  Every test asserts the plan fields its row names through gsttaco_decode_plan_fields and what decode_counters() says about
the persistent launch, and prints the plan it reached and its errors.  fp32 bound: TOL on mel (pre- and post-postnet), stop and alignment
(every row is admitted at 8 x the oracle's float32 floor <= TOL by tests/test_decoder_surface_cases.py); mixed precision: the bounds of
decoder_surface_cases' docstring against the bf16-emulating oracle."""
import gc

import numpy as np
import pytest

import decoder_surface_cases as D
from test_gpu_parity import _model, _sole_context

pytestmark = pytest.mark.gpu

KNOBS = ("GSTTACO_BILSTM_PERSIST", "GSTTACO_LEAN", "GSTTACO_ENC_WINO", "GSTTACO_WINO", "GSTTACO_WINO_SPLIT", "GSTTACO_GRAPH",
         "GSTTACO_PERSIST_DECODE", "GSTTACO_PERSIST_ROWS", "GSTTACO_FUSED_FRONT", "GSTTACO_FUSED_LSTM", "GSTTACO_PAD_DECODER")
OWN_SIZES = [c.name for c in D.CASES if c.name not in D.PERSIST_ROWS]


def _context(monkeypatch, name, shape, env=None, mixed=None):
    """A context of the row's model under ``env`` (the library reads its knobs once, at create)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    _sole_context()
    hp, w = D.model_of(name, D.is_mixed_only(name) if mixed is None else mixed)
    return _model(hp, w, shape[0], shape[1], D.TREF + 1)


def _run(m, name, shape, masked=False, forced=False, seed=None):
    """One Inference_Step of the row's inputs with injected randomness (``seed``: throughput mode instead) -> {output: array}."""
    import torch
    x = D.inputs(name, shape)
    kw = dict(seed=seed) if seed is not None else dict(prenet_masks=x.masks, attn_noise=x.noise)
    if forced:
        kw["teacher_mels"] = D.teacher(name, shape)
    else:
        kw["steps"] = shape[2]
    out = m.Inference_Step(x.tokens, x.lengths if masked else None, None, x.mels, x.mel_lengths, return_pre_mel=True, masked=masked, **kw)
    m.synchronize()
    torch.cuda.synchronize()
    mel, stop, _, align, pre = out
    assert m.handoff_error() == 0
    return {k: t.cpu().numpy() for k, t in (("mel", mel), ("stop", stop), ("align", align), ("pre_mel", pre))}


def _plan(m, name, shape, want, what="", forced=False):
    p = m.decode_plan_fields(shape[0], shape[1], forced)
    print("%s %s %s plan: %s" % (name, shape, what, " ".join("%s=%d" % kv for kv in p.items())))
    bad = {k: (p[k], v) for k, v in want.items() if p[k] != v}
    assert not bad, (name, shape, what, "plan fields (got, expected)", bad)
    return p


def _check(what, got, ref, tol=D.TOL):
    e = D.errs(got, ref)
    print("%s: max abs err %s  tolerance %.3g" % (what, " ".join("%s %.3g" % kv for kv in e.items()), tol))
    for k in D.OUTPUTS:
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (what, k)
    assert max(e.values()) <= tol, (what, e, tol)


def _check_mixed(what, got, name, shape):
    m = D.mixed_reference(name, shape)
    bad = []
    for k in D.OUTPUTS:
        assert got[k].shape == m.ref[k].shape and np.isfinite(got[k]).all(), (what, k)
        e_mean, e_max = D.mean_err(got[k], m.ref[k]), D.err(got[k], m.ref[k])
        tol_mean = D.mixed_tolerance(m.drift[k]) if k in D.LOOP_OUTPUTS else None
        tol_max = D.mixed_tolerance(m.drift_max[k]) if D.max_norm_conditioned(m, k) else D.MIXED_TOL
        print("%s %s: mean abs err %.3g (mean drift %.3g, bound %s)  max abs err %.3g (max drift %.3g, bound %.3g)" % (
            what, k, e_mean, m.drift[k], "%.3g" % tol_mean if tol_mean else "-", e_max, m.drift_max[k], tol_max))
        if (tol_mean is not None and e_mean > tol_mean) or e_max > tol_max:
            bad.append((k, e_mean, tol_mean, e_max, tol_max))
    assert not bad, (what, bad)


def _assert_bitwise(a, b, what, keys=D.OUTPUTS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k, "differs by", D.err(a[k], b[k]))


def _assert_counters(m, persist, name, shape, calls=1):
    n, on = m.decode_counters()
    if persist:
        assert on == 1 and n >= calls, (name, shape, "the persistent decode launch was not taken", n, on, m.last_message())
    else:
        assert n == 0, (name, shape, "the persistent decode launch was taken", n, on)


def _row_shape(monkeypatch, name, shape):
    """One (row, shape): the default context against the oracle with its plan and counters; a persistent call again under
    GSTTACO_PERSIST_DECODE=0, bitwise."""
    c = D.BY_NAME[name]
    want = c.plan[shape]
    only = D.is_mixed_only(name)
    masked = bool(c.lengths and shape in c.lengths)
    runs = {}
    for persist_env in (("1", "0") if want["persist"] else ("1",)):
        m = _context(monkeypatch, name, shape, {"GSTTACO_PERSIST_DECODE": persist_env})
        on = persist_env == "1"
        _plan(m, name, shape, want if on else {"persist": 0, "persist_bf16": 0, "pj_tiles": want["pj_tiles"], "dec_padded": want["dec_padded"]},
              "GSTTACO_PERSIST_DECODE=" + persist_env)
        runs[persist_env] = [_run(m, name, shape)]
        calls = 1
        if masked:
            runs[persist_env].append(_run(m, name, shape, masked=True))
            calls = 2
        _assert_counters(m, bool(want["persist"]) and on, name, shape, calls)
        del m
        gc.collect()
    got = runs["1"]
    if only:
        _check_mixed("%s %s bf16" % (name, shape), got[0], name, shape)
    else:
        _check("%s %s fp32" % (name, shape), got[0], D.reference(name, shape).ref)
    if masked:
        _check("%s %s masked" % (name, shape), got[1], D.reference(name, shape, True).ref)
        tl = D.inputs(name, shape).lengths
        for b, n in enumerate(tl):
            assert not got[1]["align"][b][:, n:].any()
    if "0" in runs:
        for a, b, what in zip(runs["1"], runs["0"], ("", " masked")):
            _assert_bitwise(a, b, "%s %s%s: the persistent launch against the launch path" % (name, shape, what))
    return got[0]


# ---------------------------------------------------------------------------------------------------- (a) the persistent launch
@pytest.mark.parametrize("name,shape", [(n, s) for n in D.PERSIST_ROWS for s in D.BY_NAME[n].shapes], ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_persistent_rows_match_the_oracle_and_the_launch_path_bitwise(monkeypatch, name, shape):
    _row_shape(monkeypatch, name, shape)


def test_hashed_randomness_is_bitwise_between_the_two_paths_at_42_tiles(monkeypatch):
    """Seeded throughput mode (keep decisions hashed from the seed, no mask tensor read) on the full-size r = 5 row."""
    name, shape = "p80x5_sma_full", (32, 23, 6)
    runs = {}
    for env in ("1", "0"):
        m = _context(monkeypatch, name, shape, {"GSTTACO_PERSIST_DECODE": env})
        runs[env] = [_run(m, name, shape, seed=4242), _run(m, name, shape, seed=4243)]
        _assert_counters(m, env == "1", name, shape)
        del m
        gc.collect()
    for a, b in zip(runs["1"], runs["0"]):
        _assert_bitwise(a, b, "hashed randomness: the persistent launch against the launch path")
    assert not np.array_equal(runs["1"][0]["pre_mel"], runs["1"][1]["pre_mel"])          # (the seed did change the trajectory)


def test_graph_replay_is_the_eager_run_at_81_tiles(monkeypatch):
    """GSTTACO_GRAPH=1 (captured at the first call, replayed at the second) against GSTTACO_GRAPH=0, bitwise."""
    name, shape = "p128x8", (16, 21, 6)
    runs = {}
    for env in ("1", "0"):
        m = _context(monkeypatch, name, shape, {"GSTTACO_GRAPH": env})
        runs[env] = [_run(m, name, shape), _run(m, name, shape)]
        assert (m.graph_cache_size() > 0) == (env == "1")
        _assert_counters(m, True, name, shape)
        del m
        gc.collect()
    _check("%s %s graph" % (name, shape), runs["1"][1], D.reference(name, shape).ref)
    for r in (runs["1"][1], runs["0"][0], runs["0"][1]):
        _assert_bitwise(runs["1"][0], r, "graph replay against the eager run")


# ---------------------------------------------------------------------------------------------------- (b) own sizes
@pytest.mark.parametrize("name", OWN_SIZES)
def test_own_size_rows_match_the_oracle_and_take_their_plan(monkeypatch, name):
    c = D.BY_NAME[name]
    for shape in c.shapes:
        got = _row_shape(monkeypatch, name, shape)
        if c.plan[shape]["fused"]:
            # the lean kernels restate the general bodies with K fixed at compile time: the decode loop is bitwise the same
            # (tests/test_gpu_parity.py holds that at the reference's sizes)
            m = _context(monkeypatch, name, shape, {"GSTTACO_LEAN": "0"})
            _plan(m, name, shape, dict(fused=1, lean_x0=0, lean_x1=0, lean_rec=0, lean_proj=0, fuse12=0, persist=0), "GSTTACO_LEAN=0")
            general = _run(m, name, shape)
            _assert_counters(m, False, name, shape)
            del m
            gc.collect()
            _check("%s %s GSTTACO_LEAN=0" % (name, shape), general, D.reference(name, shape).ref)
            _assert_bitwise(got, general, "%s %s: lean against general kernels" % (name, shape), D.LOOP_OUTPUTS)


@pytest.mark.parametrize("name", [c.name for c in D.CASES if c.mixed == "also"])
def test_own_size_row_under_mixed_precision(monkeypatch, name):
    c = D.BY_NAME[name]
    for shape in c.shapes:
        m = _context(monkeypatch, name, shape, mixed=True)
        p = _plan(m, name, shape, dict(persist=0, dec_padded=0, fused=1, z0=1), "Use_Mixed_Precision")
        assert p["lean_rec"] == 0          # (the recurrent k-block counts are the fp32 row's)
        got = _run(m, name, shape)
        _assert_counters(m, False, name, shape)
        del m
        gc.collect()
        _check_mixed("%s %s mixed" % (name, shape), got, name, shape)


@pytest.mark.parametrize("name", [c.name for c in D.CASES if c.forced])
def test_own_size_row_teacher_forced(monkeypatch, name):
    c = D.BY_NAME[name]
    for shape in c.shapes:
        m = _context(monkeypatch, name, shape)
        want = {k: v for k, v in c.plan[shape].items() if k != "fuse12"}
        _plan(m, name, shape, dict(want, persist=0), "forced", forced=True)
        got = _run(m, name, shape, forced=True)
        _assert_counters(m, False, name, shape)
        del m
        gc.collect()
        _check("%s %s forced" % (name, shape), got, D.reference(name, shape, forced=True).ref)
