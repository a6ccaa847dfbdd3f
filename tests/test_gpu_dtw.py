"""GPU tests of the free-run metric: gsttaco_mel_dtw (csrc/dtw.hip) against the float64 restatement of tests/dtw_cases.py -- cost, path
length and path per case --, its entry-point contract straight through the C ABI, non-finite propagation, and Evaluate_Free end to end
on two synthetic wavs."""
import ctypes

import numpy as np
import pytest

import audio_cases as C
import dtw_cases as D
from gst_tacotron_amd import evaluate, synthetic

pytestmark = pytest.mark.gpu

RTOL = D.RTOL


def _ptr(t, offset_bytes=0):
    return ctypes.c_void_p(t.data_ptr() + offset_bytes) if t is not None else None


def _np(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _close(got, want, rtol=RTOL):
    """|got - want| <= rtol * |want| element by element (no absolute slack: an exact 0 must come back as 0)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64
    return bool((np.abs(got - want) <= rtol * np.abs(want)).all())


def _model(case, max_batch=4):
    """A context with the case's Mel_Dim, Max_Abs_Mel and Max_Step.  No Restore: the entry needs no weights."""
    from gst_tacotron_amd.model import GST_Tacotron
    return GST_Tacotron(hyper_parameters=D.case_hp(case), max_batch=max_batch, max_tokens=8, max_ref_frames=4, max_wav_seconds=0.0)


def _check_path_against_costs(cost, n, path, Cs, shapes):
    """Independently of the oracle's path: every returned path is a warping path and the float64 sum of the oracle's C along it is the
    returned cost."""
    for b, (Lx, Ly) in enumerate(shapes):
        assert (path[b, n[b]:] == -1).all()
        if Lx == 0 or Ly == 0:
            assert cost[b] == 0.0 and n[b] == 0
            continue
        cells = path[b, :n[b]]
        assert D.path_is_valid(cells, Lx, Ly), (b, cells)
        along = np.float64(Cs[b][cells[:, 0], cells[:, 1]].sum())
        assert abs(along - cost[b]) <= RTOL * abs(along), (b, along, cost[b])


# ---------------------------------------------------------------------------------------------------- 1. the kernel, case by case
@pytest.mark.parametrize("name", D.NAMES)
def test_mel_dtw_equals_the_float64_restatement(name):
    """Mel_DTW on the case's tensors with NaN in every frame beyond a row's length.  Both sides are double and differ by FMA contraction
    and summation order (bound: dtw_cases.RTOL); tests/test_dtw_cases.py shows every choice on the path is decided by at least 1e-9
    relative, so the path is compared exactly."""
    c = D.CASES[name]
    x, xl, y, yl = D.case_inputs(name)
    want_cost, want_n, want_path, Cs, _ = D.case_reference(name)
    m = _model(c)
    px, py = D.nan_padded(x, xl), D.nan_padded(y, yl)
    args = (px, np.array(xl), py, np.array(yl), c.n_ceps)
    cost, n, path = _np(*m.Mel_DTW(*args, return_path=True))
    rel = np.abs(cost - want_cost) / np.where(want_cost != 0, np.abs(want_cost), 1.0)
    print(name, "cost", cost, "max relative error vs float64", rel.max(), "bound", RTOL, "path_len", n)
    assert cost.dtype == np.float64 and n.dtype == np.int32 and path.dtype == np.int32
    assert path.shape == (len(c.shapes), c.Tx + c.Ty - 1, 2)
    assert _close(cost, want_cost), (cost, want_cost)
    assert np.array_equal(n, want_n)
    assert np.array_equal(path, want_path)
    _check_path_against_costs(cost, n, path, Cs, c.shapes)
    if c.kind.startswith("identical"):
        assert (cost == 0.0).all()
    again = _np(*m.Mel_DTW(*args, return_path=True))
    assert np.array_equal(again[0], cost) and np.array_equal(again[1], n) and np.array_equal(again[2], path)
    plain = m.Mel_DTW(*args)
    assert len(plain) == 2
    plain = _np(*plain)
    assert np.array_equal(plain[0], cost) and np.array_equal(plain[1], n)


def test_repeated_frames_tie_exactly_and_take_the_diagonal_first():
    """y = x with every frame doubled: the two sides' features of equal frames are bitwise equal, so the cost is exactly 0 and every
    choice on the way is an exact tie -- decided by the fixed rule, as the restatement decides it."""
    c = D.CASES["generic_noise"]
    x = np.array(D.case_inputs("generic_noise")[0][:, :9])
    y = np.repeat(x, 2, axis=1)
    m = _model(c)
    cost, n, path = _np(*m.Mel_DTW(x, None, y, None, c.n_ceps, return_path=True))
    want_cost, want_n, want_path = D.dtw_reference(x, None, y, None, D.case_hp(c), c.n_ceps)
    assert cost[0] == 0.0 and want_cost[0] == 0.0 and n[0] == 18
    assert np.array_equal(n, want_n) and np.array_equal(path, want_path)


# ---------------------------------------------------------------------------------------------------- 2. the entry point
def test_mel_dtw_entry_point_contract():
    """Straight through the C ABI into NaN / sentinel-filled buffers one row longer than needed: every element of the B rows is
    written, nothing behind them; a reference passed as y + mel_dim with its stride equals the contiguous copy bitwise; NULL, too
    long and negative lengths; the documented error codes."""
    import torch
    name = "wave_edge_noise"
    c = D.CASES[name]
    x, xl, y, yl = D.case_inputs(name)
    want_cost, want_n, want_path, _, _ = D.case_reference(name)
    hp = D.case_hp(c)
    m = _model(c, max_batch=2)
    B, Tx, Ty, M = len(c.shapes), c.Tx, c.Ty, c.mel
    dev = lambda a, dt=torch.float32: torch.as_tensor(np.array(a), dtype=dt).to(m.device)
    t = {"x": dev(D.nan_padded(x, xl)), "y": dev(D.nan_padded(y, yl)), "xl": dev(xl, torch.int32), "yl": dev(yl, torch.int32)}
    lib, h = m.ctx.lib, m.ctx.handle
    rows = Tx + Ty - 1

    def fresh():
        return (torch.full((B + 1,), float("nan"), dtype=torch.float64, device=m.device),
                torch.full((B + 1,), -7, dtype=torch.int32, device=m.device),
                torch.full((B + 1, rows, 2), -7, dtype=torch.int32, device=m.device))

    def call(out, x="x", y="y", xl="xl", yl="yl", xs=0, ys=0, B=B, Tx=Tx, Ty=Ty, n_ceps=c.n_ceps, cost=True, n=True, path=True,
             y_off=0):
        g = lambda k: _ptr(t[k]) if k else None
        yp = _ptr(t[y], y_off) if y else None
        return lib.gsttaco_mel_dtw(h, g(x), g(xl), xs, yp, g(yl), ys, B, Tx, Ty, n_ceps, _ptr(out[0]) if cost else None,
                                   _ptr(out[1]) if n else None, _ptr(out[2]) if path else None, m._stream())
    out = fresh()
    assert call(out) == 0
    cost, n, path = _np(*out)
    assert _close(cost[:B], want_cost) and np.array_equal(n[:B], want_n) and np.array_equal(path[:B], want_path)
    assert np.isnan(cost[B]) and n[B] == -7 and (path[B] == -7).all()
    # path NULL: the same cost and length, the path buffer untouched
    out2 = fresh()
    assert call(out2, path=False) == 0
    c2, n2, p2 = _np(*out2)
    assert np.array_equal(c2[:B], cost[:B]) and np.array_equal(n2[:B], n[:B]) and (p2 == -7).all() and np.isnan(c2[B])
    # explicit strides equal to the default
    out3 = fresh()
    assert call(out3, xs=Tx * M, ys=Ty * M) == 0
    assert all(np.array_equal(a[:B], b[:B]) and np.array_equal(a[B:], b[B:], equal_nan=True) for a, b in zip(_np(*out3), (cost, n, path)))
    # the reference behind a prepended frame (the mels_for_gst layout): y + mel_dim with the batch stride of the larger tensor
    big = torch.full((B, Ty + 1, M), float("nan"), dtype=torch.float32, device=m.device)
    big[:, 1:] = t["y"]
    t["big"] = big
    out4 = fresh()
    assert call(out4, y="big", y_off=4 * M, ys=(Ty + 1) * M) == 0
    assert all(np.array_equal(a[:B], b[:B]) and np.array_equal(a[B:], b[B:], equal_nan=True) for a, b in zip(_np(*out4), (cost, n, path)))
    got = _np(*m.Mel_DTW(t["x"], t["xl"], big[:, 1:], t["yl"], c.n_ceps, return_path=True))     # (the same view through the model)
    assert all(np.array_equal(a, b[:B]) for a, b in zip(got, (cost, n, path)))
    # lengths NULL = T; beyond T and below 0 are clipped (on the finite tensors: every frame is read)
    t["xf"], t["yf"] = dev(x), dev(y)
    full = D.dtw_reference(x, None, y, None, hp, c.n_ceps)
    out5 = fresh()
    assert call(out5, x="xf", y="yf", xl=None, yl=None) == 0
    c5, n5, p5 = _np(*out5)
    assert _close(c5[:B], full[0]) and np.array_equal(n5[:B], full[1]) and np.array_equal(p5[:B], full[2])
    odd_x, odd_y = np.array([Tx + 9, 5], np.int32), np.array([-3, Ty + 1], np.int32)
    t["ox"], t["oy"] = dev(odd_x, torch.int32), dev(odd_y, torch.int32)
    clipped = D.dtw_reference(x, odd_x, y, odd_y, hp, c.n_ceps)
    out6 = fresh()
    assert call(out6, x="xf", y="yf", xl="ox", yl="oy") == 0
    c6, n6, p6 = _np(*out6)
    assert _close(c6[:B], clipped[0]) and np.array_equal(n6[:B], clipped[1]) and np.array_equal(p6[:B], clipped[2])
    assert c6[0] == 0.0 and n6[0] == 0 and (p6[0] == -1).all() and n6[1] >= Ty
    # errors
    out7 = fresh()
    for k in ("x", "y"):
        assert call(out7, **{k: None}) == -1 and "null" in m.last_message()
    assert call(out7, cost=False) == -1 and call(out7, n=False) == -1
    assert call(out7, B=0) == -1 and call(out7, Tx=0) == -1 and call(out7, Ty=0) == -1
    assert call(out7, n_ceps=-1) == -1 and call(out7, n_ceps=M) == -1 and "n_ceps" in m.last_message()
    assert call(out7, xs=-1) == -1
    assert call(out7, B=B + 1) == -5                                            # beyond max_batch
    assert call(out7, Tx=D.MAX_STEP + 1) == -5 and call(out7, Ty=D.MAX_STEP + 1) == -5      # beyond Max_Step
    c7, n7, p7 = _np(*out7)
    assert np.isnan(c7).all() and (n7 == -7).all() and (p7 == -7).all()         # (a refused call writes nothing)
    m.synchronize()


def test_a_non_finite_frame_spoils_its_own_row_only():
    """A NaN (or an infinity, which is not clipped into range) in a used frame of the last row: that row's cost is non-finite, every
    other row's outputs are bitwise what they were, and the call returns."""
    name = "ragged_noise"
    c = D.CASES[name]
    x, xl, y, yl = D.case_inputs(name)
    m = _model(c)
    px, py = D.nan_padded(x, xl), D.nan_padded(y, yl)
    cost, n, path = _np(*m.Mel_DTW(px, np.array(xl), py, np.array(yl), c.n_ceps, return_path=True))
    last = len(c.shapes) - 1
    assert np.isfinite(cost).all() and xl[last] > 3 and yl[last] > 3
    for side, value in (("x", np.nan), ("y", np.nan), ("x", np.inf), ("y", -np.inf)):
        bx, by = np.array(px), np.array(py)
        (bx if side == "x" else by)[last, 3, 5] = value
        got = _np(*m.Mel_DTW(bx, np.array(xl), by, np.array(yl), c.n_ceps, return_path=True))
        assert not np.isfinite(got[0][last]), (side, value, got[0])
        assert np.array_equal(got[0][:last], cost[:last]) and np.array_equal(got[1][:last], n[:last])
        assert np.array_equal(got[2][:last], path[:last])
        assert 0 <= got[1][last] <= c.Tx + c.Ty - 1
        plain = _np(*m.Mel_DTW(bx, np.array(xl), by, np.array(yl), c.n_ceps))
        assert not np.isfinite(plain[0][last]) and np.array_equal(plain[0][:last], cost[:last])


# ---------------------------------------------------------------------------------------------------- 3. Evaluate_Free
def test_evaluate_free_end_to_end_on_two_synthetic_wavs():
    """synthetic.tiny_hp() (GST, r = 2) on two short two-tone signals, free running under per-utterance seeds: ``per_utterance`` is
    ``combine_free`` of a Mel_DTW recomputed from the returned mels and report, the cost is the restatement's on the read-back mels,
    the path is a warping path with that cost (not compared cell by cell: untrained weights may emit repeated frames, exact ties
    whose order is the device's), and the same seeds give the same numbers."""
    from gst_tacotron_amd import weights
    from gst_tacotron_amd.model import GST_Tacotron, REPORT_FIELDS
    hp = synthetic.tiny_hp(max_step=64)
    case = C.Case("tiny", 33, 64, 16, 16, 4)
    assert all(hp["Sound"][k] == v for k, v in case.sound.items())
    wavs = [C.signal(case, 640, 21), C.signal(case, 420, 22)]
    sentences = ["Hi there.", "Ok"]
    m = GST_Tacotron(hyper_parameters=hp, max_batch=2, max_tokens=16, max_ref_frames=64, max_wav_seconds=1.0)
    m.Restore(weights=weights.synthetic_weights(hp, seed=4))
    seeds = [11, 2 ** 40 + 5]
    res = m.Evaluate_Free(sentences, wavs, seeds=seeds)
    assert set(res) == {"mcd", "mcd_frames", "per_utterance", "report", "mel_lengths", "ref_lengths", "mels", "ref_mels"}
    per, rep = res["per_utterance"], res["report"]
    S = hp["Max_Step"] // hp["Step_Reduction"]
    assert per.shape == (2, len(evaluate.FREE_FIELDS)) and per.dtype == np.float64 and np.isfinite(per).all()
    assert rep.shape == (2, len(REPORT_FIELDS)) and rep.dtype == np.int32
    frames, ref_len = res["mel_lengths"], res["ref_lengths"]
    assert np.array_equal(frames, rep[:, REPORT_FIELDS.index("frames")]) and (frames >= 2).all() and (frames <= 64).all()
    fm, fl = _np(*m.Mel_Generate(wavs, 15))
    assert ref_len.tolist() == fl.tolist() and ref_len[0] > ref_len[1] > 2
    mels, ref = _np(res["mels"], res["ref_mels"])
    assert mels.shape == (2, 64, 16) and np.array_equal(ref, fm[:, 1:])
    cost, n, path = _np(*m.Mel_DTW(res["mels"], frames, res["ref_mels"], ref_len, return_path=True))
    want = evaluate.combine_free(cost, n, frames, ref_len, rep[:, 0], S)
    assert np.array_equal(per, want)
    assert res["mcd"] == per[:, 0].mean() and res["mcd_frames"] == per[:, 1].sum() / per[:, 2].sum() and res["mcd"] > 0
    ref_cost, ref_n, _, Cs, _ = D.dtw_reference(mels, frames, ref, ref_len, hp, 13, with_tables=True)
    print("Evaluate_Free: mcd", res["mcd"], "per utterance", per[:, 0], "cost vs float64 rel", np.abs(cost - ref_cost) / ref_cost)
    assert _close(cost, ref_cost)
    _check_path_against_costs(cost, n, path, Cs, list(zip(frames.tolist(), ref_len.tolist())))
    again = m.Evaluate_Free(sentences, wavs, seeds=seeds)
    assert np.array_equal(again["per_utterance"], per) and again["mcd"] == res["mcd"] and again["mcd_frames"] == res["mcd_frames"]
    assert np.array_equal(again["report"], rep) and np.array_equal(_np(again["mels"])[0], mels)
    # mels given as arrays: the same numbers as from the wavs
    targets = [fm[i, 1:1 + int(fl[i])] for i in range(2)]
    from_arrays = m.Evaluate_Free(sentences, targets, seeds=seeds)
    assert np.array_equal(from_arrays["per_utterance"], per)
    # other coefficients, another number; the mel channels themselves too
    assert m.Evaluate_Free(sentences, targets, seeds=seeds, n_ceps=0)["mcd"] != res["mcd"]
    with pytest.raises(ValueError, match="one target"):
        m.Evaluate_Free(sentences, wavs[:1])
    with pytest.raises(ValueError, match="sets"):
        m.Evaluate_Free(sentences, wavs, teacher_mels=fm)
