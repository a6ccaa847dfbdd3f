"""CPU: the table of tests/serving_cases.py is sound (no GPU involved: these are properties of the calls, of the two oracles and of the
order the calls stand in, not of the kernels)."""
import numpy as np
import pytest

import decoder_surface_cases as D
import serving_cases as S

ORACLE_ITEMS = [(n, i) for n, i in S.ITEMS if S.has_oracle(n, S.BY_NAME[n].calls[i]) and i not in [b for _, b in S.repeats(n)]]
# (calls shared between the launch-path sequences and fp32_sma have the same inputs and the same model: admitted once)
_SEEN = {}
ADMISSION = [(n, i) for n, i in ORACLE_ITEMS
             if _SEEN.setdefault((tuple(sorted(S.BY_NAME[n].hp.items())), S.signature(S.BY_NAME[n].calls[i])), (n, i)) == (n, i)]


# ---------------------------------------------------------------------------------------------------- admission
@pytest.mark.parametrize("seq,i", ADMISSION, ids=lambda v: str(v))
def test_calls_are_admitted_by_the_oracle_alone(seq, i):
    """8 x the float32 floor is at most TOL on every output: the GPU bound is TOL on every fp32 call with injected randomness.  A
    call that fails here is replaced, never widened."""
    c = S.BY_NAME[seq].calls[i]
    r = S.reference(seq, i)
    print(seq, i, c.entry, (c.B, c.Tv, c.Tref, c.steps), "float32 oracle against float64:", {k: "%.3g" % v for k, v in r.floor.items()},
          "scale", {k: "%.3g" % v for k, v in r.scale.items()})
    assert set(r.ref) == set(S.outputs_of(c)) - {"durations"}
    hp, _ = S.model_of(seq)
    mel, rr = hp["Sound"]["Mel_Dim"], hp["Step_Reduction"]
    if c.entry in S.DECODE_ENTRIES:
        assert r.ref["mel"].shape == r.ref["pre_mel"].shape == (c.B, c.steps * rr, mel)
        assert r.ref["stop"].shape == (c.B, c.steps) and r.ref["align"].shape == (c.B, c.steps, c.Tv)
    for k, v in r.ref.items():
        assert np.isfinite(v).all() and r.scale[k] > 0.01, k
        assert S.FLOOR_FACTOR * r.floor[k] <= S.TOL, (k, r.floor[k])


def test_launch_path_sequences_share_the_calls_of_fp32_sma():
    """fp32_launch and fp32_front4 are calls of fp32_sma on the same model under a knob: same inputs, same oracle."""
    sma = S.BY_NAME["fp32_sma"]
    for name, idx in (("fp32_launch", (0, 1, 2, 4, 8, 7)), ("fp32_front4", (0, 1, 2))):
        s = S.BY_NAME[name]
        assert s.hp == sma.hp and s.capacity == sma.capacity and len(s.env) == 1
        assert [S.signature(c) for c in s.calls] == [S.signature(sma.calls[j]) for j in idx]


# ---------------------------------------------------------------------------------------------------- capacity
@pytest.mark.parametrize("seq", [s.name for s in S.SEQUENCES])
def test_every_call_fits_the_capacity_and_only_the_one_meant_to_equals_it(seq):
    s = S.BY_NAME[seq]
    hp, _ = S.model_of(seq)
    steps_max = hp["Max_Step"] // hp["Step_Reduction"]
    for i, c in enumerate(s.calls):
        fresh = S.fresh_capacity(c)
        assert all(a <= b for a, b in zip(fresh, s.capacity)), (seq, i, fresh, s.capacity)
        assert (fresh == s.capacity) == (i == s.full), (seq, i, "equals the capacity", fresh)
        if c.entry in S.DECODE_ENTRIES:
            assert 4 <= c.steps <= 8 and c.steps <= steps_max, (seq, i)
        elif c.entry in ("vocoder", "postnet"):
            assert c.steps <= steps_max * hp["Step_Reduction"], (seq, i)
        if c.lengths is not None:
            assert len(c.lengths) == c.B and c.lengths[0] == c.Tv and all(1 <= n <= c.Tv for n in c.lengths), (seq, i)
            assert len(set(c.lengths)) > 1
        assert c.why
    # a decode sequence opens with a call far below the capacity: what differs there is the capacity's doing alone (the modules
    # sequence runs large then small: its first call is the longest)
    if s.kind == "decoder":
        assert 4 * s.calls[0].B <= s.capacity[0] and 2 * s.calls[0].Tv <= s.capacity[1]


# ---------------------------------------------------------------------------------------------------- coverage
def _dim(c, d):
    return {"B": c.B, "Tv": c.Tv, "steps": c.steps, "Tref": c.Tref}[d]


@pytest.mark.parametrize("seq", [s.name for s in S.SEQUENCES])
def test_sequences_hold_the_transitions_they_claim(seq):
    s = S.BY_NAME[seq]
    calls = s.calls
    # a larger call directly before a smaller one, in each dimension the sequence names
    for d in s.shrinks:
        pairs = [(i, i + 1) for i in range(len(calls) - 1)
                 if (calls[i].entry == calls[i + 1].entry or s.kind == "decoder") and _dim(calls[i], d) > _dim(calls[i + 1], d) > 0]
        assert pairs, (seq, "no call directly behind one that is larger in", d)
    # the first call on the context comes back later, directly behind a call that is larger in rows and in tokens
    rep = S.repeats(seq)
    if s.kind == "decoder":
        again = [b for a, b in rep if a == 0]
        assert again, (seq, "the first call is not repeated")
        assert any(calls[b - 1].B > calls[b].B and calls[b - 1].Tv > calls[b].Tv for b in again)
        assert calls[0].rand == "injected" and calls[0].entry == "step"        # (the oracle sees the first call)
    else:
        assert rep and all(calls[a].entry == "step" for a, _ in rep)
        # the shared segments: a module call between two equal Inference_Steps, for the encoder and for the vocoder
        for entry in ("encode", "vocoder"):
            assert any(any(calls[k].entry == entry for k in range(a + 1, b)) for a, b in rep), (seq, entry)
    # every form the sequence names is reached by some call's plan
    for form in s.reaches:
        assert any(S.FORMS[form](s, c) for c in calls), (seq, "reaches no", form)


def test_plans_are_what_the_predicates_give_for_the_table_numbers():
    """The ``persist`` field of every decode call against gt_persist_decode_supported's inequalities by the call's OWN numbers
    (decoder_surface_cases.grid_inequalities): a 5-row call on a 128-row context must take a 5-row context's plan."""
    for s in S.SEQUENCES:
        for i, c in enumerate(s.calls):
            if s.kind == "decoder":
                assert c.entry in S.DECODE_ENTRIES and "persist" in c.plan
                assert c.plan["persist"] == int(S.expects_persist(s.name, c)), (s.name, i)
                assert c.plan.get("persist_bf16", 0) == int(S.expects_persist(s.name, c) and S.is_mixed(s.name)), (s.name, i)
                if "dec_padded" in c.plan:
                    assert c.plan["dec_padded"] == int(s.name == "padded_bma")
                if "mirror" in c.plan and c.plan["mirror"]:
                    assert S.is_mixed(s.name) and c.B > 32 and not c.plan["persist"]
            elif c.entry == "encode":
                couts = s.hp["enc_filters"]
                assert c.plan == dict(rows_path=int(S.enc_rows_path(couts[0], c.B, c.Tv)), f4=int(S.enc_f4(couts, c.B, c.Tv))), (s.name, i)


def test_the_forms_the_suite_must_reach_on_a_serving_context_are_all_claimed():
    claimed = {f for s in S.SEQUENCES for f in s.reaches}
    assert {"group", "one_group", "tv128", "bf16", "lsa_chain", "launch", "four_kernel"} <= claimed
    assert {"mirror_launch", "lsa_launch", "forced_launch", "hashed", "seeds", "styled", "rows_path", "f4", "gather"} <= claimed
    sma = S.BY_NAME["fp32_sma"].calls
    # the TV128 instantiation directly behind one that is not; hashed (masks_unused) directly behind injected masks; per-utterance seeds
    # (the mask tensor written again) directly behind the hashed call; the launch path between two persistent launches
    assert any(S.FORMS["tv128"](None, b) and a.Tv > 128 and a.plan["persist"] for a, b in zip(sma, sma[1:]))
    assert any(S.FORMS["hashed"](None, b) and a.rand == "injected" for a, b in zip(sma, sma[1:]))
    assert any(S.FORMS["seeds"](None, b) and S.FORMS["hashed"](None, a) for a, b in zip(sma, sma[1:]))
    assert any(a.plan["persist"] and not b.plan["persist"] and c.plan["persist"] for a, b, c in zip(sma, sma[1:], sma[2:]))
    # both M-tile counts of the one-group kernel, both group kernels' worth of rows, a partial last group
    rows = [c.B for c in sma if c.plan["persist"]]
    assert {(b + 15) // 16 for b in rows if b <= 32} == {1, 2} and any(b > 64 for b in rows) and any(32 < b <= 64 and b % 32 for b in rows)
    # mixed precision: the launch path on the mirrors directly between two launches of the bf16 kernel
    bf = S.BY_NAME["bf16"].calls
    assert any(a.plan["persist_bf16"] and b.plan.get("mirror") and c.plan["persist_bf16"] for a, b, c in zip(bf, bf[1:], bf[2:]))
    # LSA: the launch path (more than 128 tokens) directly between two launches of the chain
    ls = S.BY_NAME["lsa"].calls
    assert any(a.plan["persist"] and not b.plan["persist"] and b.Tv > S.LSA_TVMAX and c.plan["persist"] for a, b, c in zip(ls, ls[1:], ls[2:]))
    assert D.TOL == S.TOL == 5e-5 and S.BITWISE_EXCEPTIONS == ()
