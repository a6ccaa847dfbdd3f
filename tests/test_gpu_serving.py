"""GPU: one context at a service's capacity across calls of changing shape (tests/serving_cases.py).  Per sequence the SERVING context
is created once at the sequence's capacity and runs the calls in order (one live context at a time: the persistent forms need the
process's only one); per call a FRESH context of exactly the call's size (max_batch = B, max_tokens = Tv, max_ref_frames = Tref + 1, the
same hp and weights, the same knobs) makes that one call.  Asserted per call: the plan fields are the fresh context's and the table's;
every output is BITWISE the fresh context's; fp32 calls with injected randomness are within TOL of the float64 oracle on the SERVING
context's output (a stale read reproduced on both sides still fails there); equal calls of a sequence are bitwise equal on the serving
context.  A mismatch says which outputs differ, the first differing (row, step, column), and whether the sequence's first call -- which
ran on a context nothing had run on -- already differed: then the capacity alone is responsible, else stale state."""
import contextlib
import functools
import gc
import os

import numpy as np
import pytest

import decoder_surface_cases as D
import forced_cases as F
import serving_cases as S
from gst_tacotron_amd import capi
from test_gpu_parity import _model, _sole_context

pytestmark = pytest.mark.gpu

KNOBS = ("GSTTACO_BILSTM_PERSIST", "GSTTACO_LEAN", "GSTTACO_ENC_WINO", "GSTTACO_WINO", "GSTTACO_WINO_SPLIT", "GSTTACO_GRAPH",
         "GSTTACO_PERSIST_DECODE", "GSTTACO_PERSIST_ROWS", "GSTTACO_FUSED_FRONT", "GSTTACO_FUSED_LSTM", "GSTTACO_PAD_DECODER")
F4_IDS = {capi.CONV_V[k] for k in ("WINO4", "WINO4_S", "WINO4_S_X3")} | {capi.CONV_VH["WINO4_S"]}


@contextlib.contextmanager
def _knobs(env):
    """The sequence's knobs and no others (the library reads its knobs once, at create)."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _create(seq, capacity):
    _sole_context()
    with _knobs(S.BY_NAME[seq].env):
        hp, w = S.model_of(seq)
        return _model(hp, w, *capacity)


def _plan(m, c):
    """What the context says it launches for the call: the decode plan's fields; for the modules the dispatcher's kernel ids."""
    if c.entry in S.DECODE_ENTRIES:
        return m.decode_plan_fields(c.B, c.Tv, c.entry == "forced")
    if c.entry == "encode":
        ids, rows = m.encoder_variants(c.B, c.Tv)
        return dict(rows_path=int(rows), f4=int(any(v in F4_IDS for v in ids)), ids=tuple(ids))
    if c.entry == "vocoder":
        return {k: tuple(v) for k, v in m.vocoder_variants(c.B, c.steps).items()}
    if c.entry == "postnet":
        return dict(ids=tuple(m.postnet_variants(c.B, c.steps)))
    return {}


def _call(m, seq, i):
    """Call ``i`` of a sequence on context ``m`` -> {output: host array}, every output of serving_cases.outputs_of."""
    import torch
    c = S.BY_NAME[seq].calls[i]
    x = S.inputs(seq, i)
    out = {}
    if c.entry in S.DECODE_ENTRIES:
        if c.rand == "injected":
            kw = dict(prenet_masks=x.masks, attn_noise=x.noise)
        elif c.rand[0] == "seed":
            kw = dict(seed=c.rand[1])
        else:
            kw = dict(seeds=[c.rand[1] + b for b in range(c.B)])
        if c.entry == "forced":
            kw["teacher_mels"] = x.teacher
        else:
            kw["steps"] = c.steps
        mels, ml = x.mels, x.mel_lengths
        if c.entry == "styled":
            out["style"] = kw["style_embeddings"] = m.Inference_GST_Step(mels, ml)
            mels = ml = None
        mel, stop, spec, align, pre = m.Inference_Step(x.tokens, x.lengths, None, mels, ml, return_pre_mel=True, masked=c.lengths is not None,
                                                       with_vocoder=c.vocoder, **kw)
        out.update(mel=mel, stop=stop, align=align, pre_mel=pre)
        if c.vocoder:
            out["spectrogram"] = spec
        if c.entry == "forced":
            out["durations"] = m.Forced_Durations(align)
    elif c.entry == "encode":
        out["memory"] = m.encode(x.tokens, x.lengths)
    elif c.entry == "gst":
        out["style"] = m.Inference_GST_Step(x.mels, x.mel_lengths)
    elif c.entry == "vocoder":
        out["spectrogram"] = m.vocoder(x.x)
    else:
        out["mel"] = m.postnet(x.x)
    m.synchronize()
    torch.cuda.synchronize()
    assert m.handoff_error() == 0, (seq, i, m.last_message())
    if "keep_masks" in S.outputs_of(c):         # (what the hashed decisions were, written out now: masks_lazy is the LAST decode's)
        out["keep_masks"], out["noise"] = m.debug_randomness(c.steps, c.B, c.Tv)
    return {k: out[k] if isinstance(out[k], np.ndarray) else out[k].cpu().numpy() for k in S.outputs_of(c)}


def _once(fn):
    """functools.lru_cache that keeps a failure too: a sequence that failed is not run again for every item that asks for it."""
    memo = {}

    @functools.wraps(fn)
    def wrapper(*key):
        if key not in memo:
            try:
                memo[key] = (fn(*key), None)
            except Exception as e:              # (kept and raised again, for this item and every later one)
                memo[key] = (None, e)
        value, failure = memo[key]
        if failure is not None:
            raise failure
        return value
    return wrapper


@_once
def _serving(seq):
    """The sequence on ONE context of its capacity -> per call (outputs, plan, persistent decode launches enqueued by the call)."""
    s = S.BY_NAME[seq]
    m = _create(seq, s.capacity)
    runs = []
    for i, c in enumerate(s.calls):
        plan = _plan(m, c)
        before = m.decode_counters()[0]
        out = _call(m, seq, i)
        n, on = m.decode_counters()
        if any(k.plan.get("persist") for k in s.calls):
            assert on == 1, (seq, i, "the context no longer uses the persistent decode launch", m.last_message())
        runs.append((out, plan, n - before))
    del m
    gc.collect()
    return runs


@_once
def _fresh(seq, i):
    """Call ``i`` alone on a context of exactly its size -> (outputs, plan)."""
    c = S.BY_NAME[seq].calls[i]
    m = _create(seq, S.fresh_capacity(c))
    plan = _plan(m, c)
    out = _call(m, seq, i)
    del m
    gc.collect()
    return out, plan


def _first_difference(seq, i, k, a, b):
    """'row r, step s, column c' of the first element in which output ``k`` of two runs of a call differs."""
    c = S.BY_NAME[seq].calls[i]
    if a.shape != b.shape:
        return "shapes %s and %s" % (a.shape, b.shape)
    idx = tuple(int(v) for v in np.argwhere(a != b)[0])
    if k in ("keep_masks", "noise"):            # ([steps, 2, B, P] and [steps, B, Tv])
        return "step %d, row %d, index %s (%r against %r; %d of %d elements differ)" % (idx[0], idx[-2], idx, a[idx], b[idx], int((a != b).sum()), a.size)
    r = S.model_of(seq)[0]["Step_Reduction"]
    row = idx[0]
    if k in ("mel", "pre_mel", "spectrogram") and c.entry in S.DECODE_ENTRIES:
        step, col = idx[1] // r, "frame %d column %d" % (idx[1], idx[2])
    elif len(idx) == 3:
        step, col = idx[1], "column %d" % idx[2]
    elif k == "stop":
        step, col = idx[1], "-"
    else:
        step, col = "-", "column %d" % idx[-1]
    return "row %s, step %s, %s (%r against %r; %d of %d elements differ, by at most %.3g)" % (
        row, step, col, a[idx], b[idx], int((a != b).sum()), a.size, D.err(a, b))


def _differing(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


def _diagnosis(seq, i):
    """Capacity or stale state?  The sequence's first call ran on a context nothing had run on: if IT differs from its fresh context
    the capacity alone is responsible; if it does not, what differs later is state an earlier call left behind."""
    if i == 0:
        return "this IS the first call on its context: the capacity alone is responsible, nothing was stale"
    first = _differing(_serving(seq)[0][0], _fresh(seq, 0)[0])
    if first:
        return "the first call on the context already differs (%s): the capacity is responsible, with or without stale state" % ", ".join(first)
    return "the first call on the context is bitwise its fresh context's: stale state, not capacity (calls 0 .. %d ran before)" % (i - 1)


def _describe(seq, i):
    c = S.BY_NAME[seq].calls[i]
    return "%s call %d (%s %dx%d Tref %d steps %d, %s%s) on capacity %s" % (
        seq, i, c.entry, c.B, c.Tv, c.Tref, c.steps, c.rand, ", masked" if c.lengths else "", S.BY_NAME[seq].capacity)


# ---------------------------------------------------------------------------------------------------- the serving context against a fresh one
@pytest.mark.parametrize("seq,i", S.ITEMS, ids=lambda v: str(v))
def test_a_call_on_the_serving_context_is_the_call_on_a_fresh_context(seq, i):
    s = S.BY_NAME[seq]
    c = s.calls[i]
    got, plan, launches = _serving(seq)[i]
    alone, plan_alone = _fresh(seq, i)
    what = _describe(seq, i)
    print(what, "plan:", " ".join("%s=%s" % kv for kv in plan.items()), "| persistent decode launches enqueued:", launches)
    # the plan: the fresh context's, and the table's
    bad = {k: (plan.get(k), plan_alone.get(k)) for k in set(plan) | set(plan_alone) if plan.get(k) != plan_alone.get(k)}
    assert not bad, (what, "plan fields (serving, fresh)", bad, "the plan reads the capacity, not the call")
    bad = {k: (plan[k], v) for k, v in c.plan.items() if plan[k] != v}
    assert not bad, (what, "plan fields (got, the table's)", bad)
    if c.entry in S.DECODE_ENTRIES:
        if not plan["persist"]:
            assert launches == 0, (what, "the persistent decode launch was taken", launches)
        elif i not in [b for _, b in S.repeats(seq)]:        # (an equal call replays its graph: nothing is enqueued)
            assert launches >= 1, (what, "the persistent decode launch was not taken")
    # the outputs: bitwise
    assert set(got) == set(alone) == set(S.outputs_of(c))
    if (seq, i) in S.BITWISE_EXCEPTIONS:
        return
    diff = _differing(got, alone)
    if diff:
        lines = ["%s: the serving context differs from a fresh context of %s in %s" % (what, S.fresh_capacity(c), ", ".join(diff))]
        lines += ["  %s: first at %s" % (k, _first_difference(seq, i, k, got[k], alone[k])) for k in diff]
        lines.append("  " + _diagnosis(seq, i))
        print("\n".join(lines))
        pytest.fail("\n".join(lines), pytrace=False)
    for k, v in got.items():
        assert np.isfinite(v).all(), (what, k, "is not finite")


# ---------------------------------------------------------------------------------------------------- the serving context against the oracle
@pytest.mark.parametrize("seq,i", [(n, i) for n, i in S.ITEMS if S.has_oracle(n, S.BY_NAME[n].calls[i])], ids=lambda v: str(v))
def test_a_call_on_the_serving_context_matches_the_oracle(seq, i):
    c = S.BY_NAME[seq].calls[i]
    got = _serving(seq)[i][0]
    ref = S.reference(seq, i).ref
    what = _describe(seq, i)
    e = {k: D.err(got[k], ref[k]) for k in ref}
    print("%s: max abs err %s  tolerance %.3g" % (what, " ".join("%s %.3g" % kv for kv in e.items()), S.TOL))
    for k in ref:
        assert got[k].shape == ref[k].shape, (what, k)
    bad = {k: v for k, v in e.items() if not v <= S.TOL}
    if bad:
        # (against the oracle alone a wrong result says nothing about its cause: the fresh context's error tells capacity / stale from a
        # kernel that is wrong at this shape on every context)
        alone = _fresh(seq, i)[0]
        e_alone = {k: D.err(alone[k], ref[k]) for k in bad}
        fresh_ok = all(v <= S.TOL for v in e_alone.values())
        pytest.fail("%s: above TOL = %.3g against the float64 oracle: %s; a fresh context of %s has %s.  %s" % (
            what, S.TOL, bad, S.fresh_capacity(c), e_alone,
            _diagnosis(seq, i) if fresh_ok else "the fresh context misses the oracle too: not a property of the serving context"),
            pytrace=False)
    if c.lengths is not None and "align" in got:
        for b, n in enumerate(c.lengths):
            assert not got["align"][b][:, n:].any(), (what, "row", b, "attends beyond its", n, "tokens")
    if c.entry == "forced":
        r = S.model_of(seq)[0]["Step_Reduction"]
        assert np.array_equal(got["durations"], F.durations(got["align"], r)), (what, "durations")


# ---------------------------------------------------------------------------------------------------- equal calls on the serving context
@pytest.mark.parametrize("seq,a,b", [(s.name, a, b) for s in S.SEQUENCES for a, b in S.repeats(s.name)], ids=lambda v: str(v))
def test_equal_calls_are_bitwise_equal_on_the_serving_context(seq, a, b):
    runs = _serving(seq)
    diff = _differing(runs[a][0], runs[b][0])
    if diff:
        lines = ["%s differs from the same call at index %d in %s" % (_describe(seq, b), a, ", ".join(diff))]
        lines += ["  %s: first at %s" % (k, _first_difference(seq, b, k, runs[b][0][k], runs[a][0][k])) for k in diff]
        lines.append("  calls %d .. %d ran between them: stale state, not capacity (the capacity is the same for both)" % (a + 1, b - 1))
        pytest.fail("\n".join(lines), pytrace=False)


def test_the_named_launch_forms_were_reached_on_a_serving_context():
    """From the plans the serving contexts reported (not the table's): group, one-group, TV128, bf16, LSA chain, launch path and
    four-kernel front end were each run on a context larger than the call."""
    reached = set()
    for s in S.SEQUENCES:
        for c, (_, plan, launches) in zip(s.calls, _serving(s.name)):
            live = c._replace(plan=plan)
            if S.fresh_capacity(c) == s.capacity:
                continue
            reached |= {f for f in s.reaches if S.FORMS[f](s, live)}
    print("reached on a serving context:", sorted(reached))
    assert {"group", "one_group", "tv128", "bf16", "lsa_chain", "launch", "four_kernel"} <= reached
