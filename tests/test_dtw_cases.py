"""CPU tests of the free-run metric's host side: the float64 restatement of gsttaco_mel_dtw and its case table (tests/dtw_cases.py), the
constants and the reduction in gst_tacotron_amd/evaluate.py, and the declared surface (header, capi, model)."""
import inspect
import os

import numpy as np
import pytest

import dtw_cases as D
from gst_tacotron_amd import capi, evaluate, hparams, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the case table
def test_the_table_holds_the_shapes_and_kinds_it_must():
    shapes = {s for c in D.CASES.values() for s in c.shapes}
    for want in ((1, 1), (1, 7), (5, 1), (37, 53), (64, 65), (65, 64), (130, 97), (3, 1100), (1100, 3)):
        assert want in shapes
    for name in ("ragged_noise", "ragged_warp"):
        c = D.CASES[name]
        assert c.shapes == ((37, 53), (0, 9), (12, 0), (20, 20)) and (c.Tx, c.Ty) == (40, 56)
    kinds = {c.kind for c in D.CASES.values()}
    assert {"noise", "warp", "identical", "beyond", "unit"} <= kinds
    tiny = synthetic.tiny_hp()["Sound"]["Mel_Dim"]
    assert {(c.mel, c.n_ceps) for c in D.CASES.values()} >= {(80, 0), (80, 13), (80, 79), (tiny, 0), (tiny, 13), (tiny, tiny - 1)}
    assert D.MAX_STEP == 1100 and all(max(c.Tx, c.Ty) <= c.max_step for c in D.CASES.values())
    for name, c in D.CASES.items():
        x, xl, y, yl = D.case_inputs(name)
        assert x.dtype == y.dtype == np.float32 and x.shape == (len(c.shapes), c.Tx, c.mel) and y.shape == (len(c.shapes), c.Ty, c.mel)
        assert np.isfinite(x).all() and np.isfinite(y).all()
        lo, hi = evaluate.mel_range(D.case_hp(c))
        assert (lo, hi) == ((-4.0, 4.0) if c.max_abs else (0.0, 1.0))
        inside = x.min() >= lo and x.max() <= hi and y.min() >= lo and y.max() <= hi
        assert inside == (c.kind != "beyond")               # (the one case in which the clip matters)
        px = D.nan_padded(x, xl)
        assert all(np.isnan(px[b, n:]).all() and np.isfinite(px[b, :n]).all() for b, n in enumerate(xl))


@pytest.mark.parametrize("name", [n for n in D.NAMES if not D.CASES[n].kind.startswith("identical")])
def test_cases_are_well_conditioned(name):
    """What admits a case for an exact path comparison: the restatement in extended precision walks the same path to a cost within
    1e-12, and at every cell of the path the chosen predecessor beats the runner-up by at least 1e-9 relative -- five decades above
    what separates two double implementations, so neither the summation order nor FMA contraction can turn a choice."""
    c = D.CASES[name]
    x, xl, y, yl = D.case_inputs(name)
    cost, n, path, Cs, Ds = D.case_reference(name)
    cost_l, n_l, path_l = D.dtw_reference(x, xl, y, yl, D.case_hp(c), c.n_ceps, dtype=np.longdouble)
    assert np.array_equal(n, n_l) and np.array_equal(path, path_l)
    rel = np.abs(cost_l - cost.astype(np.longdouble)) / np.where(cost != 0, np.abs(cost_l), 1)
    margins = [D.path_margin(Cs[b], Ds[b], [tuple(p) for p in path[b, :n[b]]]) for b in range(len(c.shapes)) if n[b]]
    print(name, "cost vs long double: max rel", float(rel.max()), "smallest on-path margin", min(margins))
    assert (rel <= 1e-12).all()
    assert min(margins) >= 1e-9
    assert (cost[n > 0] > 0).all() and np.isfinite(cost).all()


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", D.NAMES)
def test_reference_paths_are_warping_paths(name):
    c = D.CASES[name]
    cost, n, path, Cs, Ds = D.case_reference(name)
    assert cost.dtype == np.float64 and n.dtype == np.int32 and path.shape == (len(c.shapes), c.Tx + c.Ty - 1, 2)
    for b, (Lx, Ly) in enumerate(c.shapes):
        assert (path[b, n[b]:] == -1).all()
        if Lx == 0 or Ly == 0:
            assert cost[b] == 0 and n[b] == 0
            continue
        cells = path[b, :n[b]]
        assert D.path_is_valid(cells, Lx, Ly) and max(Lx, Ly) <= n[b] <= Lx + Ly - 1
        assert (np.diff(cells[:, 0]) >= 0).all() and (np.diff(cells[:, 1]) >= 0).all()
        along = Cs[b][cells[:, 0], cells[:, 1]].sum()
        assert abs(along - cost[b]) <= 1e-12 * cost[b]
        if c.kind.startswith("identical"):
            assert cost[b] == 0.0 and n[b] == Lx == Ly and np.array_equal(cells, np.stack([np.arange(Lx)] * 2, 1))


def test_brute_force_recursion_agrees_and_pins_the_tie_rule():
    rng = np.random.default_rng(7)
    ties = 0
    for Lx in range(1, 7):
        for Ly in range(1, 7):
            for C in (rng.integers(0, 3, size=(Lx, Ly)).astype(np.float64), rng.random((Lx, Ly))):
                Dm, dirs = D.dtw_table(C)
                cells = D.walk_back(dirs)
                cost, want = D.brute_force(C)
                assert Dm[-1, -1] == cost and cells == want, (C, cells, want)
                assert D.path_is_valid(cells, Lx, Ly)
                ties += int(D.path_margin(C, Dm, cells) == 0.0)
    assert ties >= 10                                       # (the small-integer matrices are full of exact ties)
    # the rule itself: diagonal first, up only if strictly smaller, left only if strictly smaller than the best so far
    assert D.walk_back(D.dtw_table(np.zeros((2, 2)))[1]) == [(0, 0), (1, 1)]
    assert D.walk_back(D.dtw_table(np.array([[0.0, 1.0], [0.0, 1.0]]))[1]) == [(0, 0), (1, 1)]           # diagonal = left (0): diagonal
    C = np.array([[1.0, 0.0], [3.0, 1.0]])                  # up D(0,1) = 1 equals the diagonal D(0,0) = 1; left D(1,0) = 4
    assert D.walk_back(D.dtw_table(C)[1]) == [(0, 0), (1, 1)]
    C = np.array([[2.0, 0.0, 9.0], [0.0, 0.0, 1.0]])        # at (1,2): diagonal D(0,1) = 2, up D(0,2) = 11, left D(1,1) = 2 -> diagonal
    assert D.walk_back(D.dtw_table(C)[1])[-2] == (0, 1)
    # exact ties from repeated frames through the whole restatement: y = x with every frame doubled
    hp = hparams.load_hp()
    x = rng.normal(size=(1, 3, 80)).astype(np.float32)
    y = np.repeat(x, 2, axis=1)
    cost, n, path = D.dtw_reference(x, None, y, None, hp, 13)
    assert cost[0] == 0.0 and n[0] == 6 and path[0, :6].tolist() == [[0, 0], [0, 1], [1, 2], [1, 3], [2, 4], [2, 5]]
    Cm = D.local_cost(D.features(x[0], hp, 13), D.features(y[0], hp, 13))
    assert D.brute_force(Cm)[1] == [tuple(p) for p in path[0, :6]]


def test_clip_and_scale_of_the_restatement():
    hp = hparams.load_hp()
    x = np.array([[9.0] * 80, [-9.0] * 80, [4.0] * 80], np.float32)
    f = D.features(x, hp, 0)
    assert np.array_equal(f[0], f[2]) and np.array_equal(f[1], -f[2])
    # one unit of difference in every channel is g dB per channel: distance g sqrt(80) / sqrt(2)
    a, b = np.zeros((1, 80), np.float32), np.ones((1, 80), np.float32)
    want = 12.5 * np.sqrt(80.0) / np.sqrt(2.0)
    assert abs(D.local_cost(D.features(a, hp, 0), D.features(b, hp, 0))[0, 0] - want) <= 1e-12 * want
    # the orthonormal transform keeps distances except for what c0 and the dropped coefficients carried: a constant offset is all c0
    assert D.local_cost(D.features(a, hp, 79), D.features(b, hp, 79))[0, 0] <= 1e-12 * want


# ---------------------------------------------------------------------------------------------------- evaluate.py
def test_dct_basis_is_orthonormal_and_drops_c0():
    for n_ceps, M in ((13, 80), (79, 80), (1, 16), (15, 16)):
        b = evaluate.dct_basis(n_ceps, M)
        assert b.dtype == np.float64 and b.shape == (n_ceps, M)
        assert np.abs(b @ b.T - np.eye(n_ceps)).max() <= 1e-14
        assert np.abs(b.sum(axis=1)).max() <= 1e-13         # orthogonal to the constant row c0 would be
        k, m = n_ceps, M - 1
        assert b[k - 1, m] == np.sqrt(2.0 / M) * np.cos(np.pi * k * (2.0 * m + 1.0) / (2.0 * M))
    for bad in ((0, 80), (80, 80), (-1, 16)):
        with pytest.raises(ValueError):
            evaluate.dct_basis(*bad)


def test_mcd_scale_for_both_normalisations():
    hp = hparams.load_hp()
    assert hp["Sound"]["Max_Abs_Mel"] == 4
    assert evaluate.mel_range(hp) == (-4.0, 4.0) and evaluate.mcd_scale(hp) == 100.0 / 8.0 / np.sqrt(2.0)
    hp["Sound"]["Max_Abs_Mel"] = 0
    assert evaluate.mel_range(hp) == (0.0, 1.0) and evaluate.mcd_scale(hp) == 100.0 / np.sqrt(2.0)
    hp["Sound"]["Max_Abs_Mel"] = 4.1                         # the context holds a float32
    assert evaluate.mel_range(hp)[1] == float(np.float32(4.1)) and evaluate.mcd_scale(hp) == 100.0 / (2 * float(np.float32(4.1))) / np.sqrt(2.0)
    # the identity behind the scale: (10 / ln 10) sqrt(2 sum dc^2) with dc = g dv ln 10 / 20
    dv = np.array([0.3, -1.2, 0.7])
    g = 100.0 / 8.0
    usual = 10.0 / np.log(10.0) * np.sqrt(2.0 * ((g * dv * np.log(10.0) / 20.0) ** 2).sum())
    hp["Sound"]["Max_Abs_Mel"] = 4
    assert abs(usual - evaluate.mcd_scale(hp) * np.sqrt((dv ** 2).sum())) <= 1e-13 * usual


def test_combine_free():
    assert evaluate.FREE_FIELDS == ("mcd", "cost", "path_len", "frames", "ref_frames", "duration_ratio", "stop_fired")
    per = evaluate.combine_free([6.0, 0.0, 9.0], [3, 0, 2], [4, 2, 6], [5, 0, 3], [2, 1, 3], 3)
    assert per.dtype == np.float64 and per.shape == (3, 7)
    assert per.tolist() == [[2.0, 6.0, 3.0, 4.0, 5.0, 0.8, 1.0], [0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 1.0], [4.5, 9.0, 2.0, 6.0, 3.0, 2.0, 0.0]]
    s = evaluate.summarize_free(per)
    assert s == {"mcd": (2.0 + 0.0 + 4.5) / 3, "mcd_frames": 15.0 / 5.0}
    assert evaluate.summarize_free(evaluate.combine_free([0.0], [0], [2], [0], [1], 1)) == {"mcd": 0.0, "mcd_frames": 0.0}
    assert np.isnan(evaluate.combine_free([np.nan], [3], [2], [4], [1], 1)[0, 0])      # (a non-finite cost stays visible)
    with pytest.raises(ValueError):
        evaluate.combine_free([1.0, 2.0], [1], [1, 1], [1, 1], [1, 1], 2)


# ---------------------------------------------------------------------------------------------------- the declared surface
def test_new_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    assert "int gsttaco_mel_dtw(" in header and "gsttaco_mel_dtw" in capi.EXPORTED_SYMBOLS and capi.ABI_VERSION == 14
    for text in ("double* cost", "int32_t* path_len", "int64_t x_stride", "int64_t y_stride", "GSTTACO_E_CAPACITY: B > max_batch"):
        assert text in header
    from gst_tacotron_amd import build
    assert "dtw.hip" in build.SOURCES
    lib = capi.load_library()
    assert len(lib.gsttaco_mel_dtw.argtypes) == 15


def test_model_methods_exist_with_the_stated_keywords():
    from gst_tacotron_amd.model import GST_Tacotron
    p = inspect.signature(GST_Tacotron.Mel_DTW).parameters
    assert list(p)[1:] == ["mels", "mel_lengths", "ref_mels", "ref_lengths", "n_ceps", "return_path"]
    assert p["n_ceps"].default == 13 and p["return_path"].default is False
    p = inspect.signature(GST_Tacotron.Evaluate_Free).parameters
    assert list(p)[1:7] == ["sentence_List", "mel_or_wav_List", "wav_List_for_GST", "style_embeddings", "seeds", "n_ceps"]
    assert p["n_ceps"].default == 13 and all(p[k].default is None for k in ("wav_List_for_GST", "style_embeddings", "seeds"))
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in p.values())
