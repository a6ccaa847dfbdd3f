"""CPU checks of tests/style_map_cases.py: every case is admitted by a conditioning test -- each decision of the perplexity search and of
the descent falls by at least MARGIN and falls the same way in float64 and in np.longdouble, and the two precisions agree within
RTOL / 16 (the device differs from float64 by FMA contraction and summation order: rounding of the kind and size this comparison
measures, and a sixteenth leaves it room) --, the table reaches the edges it names, the 1000-step run of ``blobs120`` separates its
clusters, and the host side of the feature (symbols, export, init, signatures) is what the documents say.  A case that fails the
conditioning test is changed, not excused."""
import inspect
import os
import re

import numpy as np
import pytest

import style_map_cases as S
from gst_tacotron_amd import capi, export

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the affinities
@pytest.mark.parametrize("name", S.AFFINITY_NAMES)
def test_every_search_decision_is_decided_by_the_margin(name):
    """|Hd| against 1e-5 in every round (which, 1e-5 being above the margin, also decides every sign of Hd that was used) and with it
    the round count: so beta and search_iters are the same in both precisions and may be compared exactly on the device."""
    a, b = S.affinity_reference(name), S.affinity_reference(name, np.longdouble)
    print(name, "smallest decision margin", a["margin"], b["margin"], "rounds", a["search_iters"].min(), "..", a["search_iters"].max(),
          "beta", a["beta"].min(), "..", a["beta"].max())
    assert min(a["margin"], b["margin"]) >= S.MARGIN
    assert np.array_equal(a["search_iters"], b["search_iters"]) and np.array_equal(a["beta"], b["beta"].astype(np.float64))
    assert np.array_equal(a["beta"].astype(np.longdouble), b["beta"])           # (every beta is a double: doublings, halvings, means)
    p, q = a["p"], b["p"].astype(np.float64)
    assert np.isfinite(p).all() and (np.abs(p - q) <= S.RTOL / 16 * np.abs(q) + 2.0 ** -1022).all()
    assert np.array_equal(p, p.T) and (np.diag(p) == 0).all() and abs(p.sum() - 1) <= p.size * 2.0 ** -52


def test_the_affinity_table_reaches_the_edges_it_names():
    c = S.AFFINITY_CASES
    assert [c[n].N for n in ("n3", "n7_d1", "n63", "n64", "n65", "n255_d256", "n257_d256", "n1030")] == [3, 7, 63, 64, 65, 255, 257, 1030]
    assert c["n7_d1"].D == 1 and c["n255_d256"].D == c["n257_d256"].D == 256 and c["blobs120"].x.shape == (120, 16)
    assert [c[n].perplexity for n in ("n3", "n7_d1", "n64", "n255_d256", "dups_outlier", "three_duplicates", "blobs120")] == [1.5, 2, 5, 30, 4, 2.5, 5]
    w = c["wide_rows"]
    assert w.ldx > w.D and w.x.shape == (w.N, w.D) and not w.x.flags["C_CONTIGUOUS"]
    d = c["dups_outlier"]
    assert (d.N, d.D) == (33, 8) and np.array_equal(d.x[0], d.x[1]) and np.array_equal(d.x[0], d.x[2])
    assert np.sqrt(S.distances(d.x)[32, :32].min()) > 95
    r = S.affinity_reference("dups_outlier")
    assert r["beta"][32] < 0.1 and r["beta"].max() > 2 and (S.distances(d.x)[0, 1:3] == 0).all()      # halved, and doubled past 2
    t = S.affinity_reference("three_duplicates")
    assert (t["search_iters"][:4] == 200).all() and (t["beta"][:4] == 2.0 ** 200).all()
    # (a point whose four nearest neighbours are those duplicates -- equidistant, H >= log 4 -- runs all the rounds too)
    assert (t["search_iters"][4:] < 200).sum() >= 6 and (t["beta"][t["search_iters"] == 200] == 2.0 ** 200).all()
    assert np.allclose(t["cond"][0, 1:4], 1 / 3, rtol=1e-15) and (t["cond"][0, 4:] == 0).all()


def test_scaling_the_embeddings_leaves_every_search_bounded():
    """The row shift keeps s >= 1 whatever the data's scale: embeddings 1e6 and 1e-6 times as large end with finite beta and p."""
    x = S.AFFINITY_CASES["n64"].x
    for scale in (1e6, 1e-6):
        r = S.affinities_reference((x * scale).astype(np.float32), 5.0)
        assert np.isfinite(r["p"]).all() and np.isfinite(r["beta"]).all() and r["search_iters"].max() < 200 and abs(r["p"].sum() - 1) < 1e-12


# ---------------------------------------------------------------------------------------------------- the descent
@pytest.mark.parametrize("name", S.DESCENT_NAMES)
def test_every_descent_case_is_well_conditioned(name):
    c = S.DESCENT_CASES[name]
    a, b = S.descent_case_reference(name), S.descent_case_reference(name, np.longdouble)
    scale = float(np.abs(a["y"]).max())
    if c.iters:
        assert np.array_equal(a["decisions"], b["decisions"])
        print(name, "min|g| / max|g|", a["g_ratio"], "worst difference / max|y|",
              max(float(np.abs(a[k] - b[k].astype(np.float64)).max()) for k in ("y", "velocity", "gains")) / scale)
        assert min(a["g_ratio"], b["g_ratio"]) >= S.MARGIN
    for k in ("y", "velocity", "gains"):
        assert np.isfinite(a[k]).all() and (np.abs(a[k] - b[k].astype(np.float64)) <= S.RTOL / 16 * scale).all(), (name, k)
    assert abs(a["kl"] - b["kl"]) <= S.RTOL / 16 * abs(a["kl"])
    assert abs(a["y"].mean(axis=0)).max() <= 1e-12 * scale or not c.iters


def test_the_descent_table_reaches_the_edges_it_names():
    c = S.DESCENT_CASES
    for run in ("blobs120", "dups_outlier"):
        assert all("%s_from_%d_steps_%d" % (run, t, k) in c for t in (0, 245, 500, 990) for k in (1, 5, 10))
    x = c["blobs120_from_245_steps_10"]
    assert x.first_iter < 250 < x.first_iter + x.iters                  # crosses both switches
    e = c["early_switches_from_0_steps_10"]
    assert e.schedule == dict(stop_lying_iter=3, mom_switch_iter=4)
    # the two schedules part at step 3: the same start, other states
    plain = S.descent_reference(e.p, *e.state, 0, 10)
    assert not np.array_equal(plain["y"], S.descent_case_reference(e.name)["y"])
    pinned = S.descent_case_reference("pinned_gains")
    assert (pinned["gains"] == 0.01).any() and (pinned["gains"] > 0.01).any() and pinned["gains"].min() == 0.01
    k = c["kl_only"]
    assert k.iters == 0 and k.kl_only and np.array_equal(S.descent_case_reference("kl_only")["y"], k.state[0])
    assert c["n1030_from_0_steps_5"].p.shape[0] > 1024


def test_blobs_separate_at_every_seed():
    """1000 steps of the restatement at the defaults: every point's nearest neighbour in the map is from its own cluster, and the KL
    divergence is the recorded one up to the spread between equally valid trajectories."""
    got = []
    for seed in range(4):
        y, kl = S.blobs_run(seed)
        got.append(kl)
        assert np.isfinite(y).all() and S.purity(y, S.BLOBS_LABELS) == 1.0, seed
    print("blobs120 KL at seeds 0 .. 3:", got)
    assert len(S.BLOBS_KL) == 4 and all(min(S.BLOBS_KL) / 1.25 <= kl <= 1.25 * max(S.BLOBS_KL) for kl in got)


def test_the_descent_is_chaotic_beyond_a_few_dozen_steps():
    """Why no test compares a long run value by value: float64 and long double agree to rounding after 10 steps from t = 0 and no
    longer to RTOL after 60."""
    p = S.affinity_reference("blobs120")["p"]
    y0, v0, g0 = S.default_init(120, 0), np.zeros((120, 2)), np.ones((120, 2))
    rel = {}
    for steps in (10, 60):
        a = S.descent_reference(p, y0, v0, g0, 0, steps)["y"]
        b = S.descent_reference(p, y0, v0, g0, 0, steps, dtype=np.longdouble)["y"].astype(np.float64)
        rel[steps] = float(np.abs(a - b).max() / np.abs(a).max())
    print("float64 against long double, of max|y|:", rel)
    assert rel[10] <= S.RTOL / 16 and rel[60] > rel[10]


# ---------------------------------------------------------------------------------------------------- the host side
def test_the_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gsttaco.h")).read()
    declared = set(re.findall(r"\b(gsttaco_[a-z_0-9]+)\s*\(", header))
    for sym in ("gsttaco_style_affinities", "gsttaco_style_map"):
        assert sym in declared and sym in capi.EXPORTED_SYMBOLS
    assert capi.ABI_VERSION == 14 and "#define GSTTACO_ABI_VERSION 14" in header
    kernels = open(os.path.join(ROOT, "gst_tacotron_amd", "csrc", "kernels.h")).read()
    assert "gt_launch_style_affinities" in kernels and "gt_launch_style_map" in kernels
    from gst_tacotron_amd import build
    assert "tsne.hip" in build.SOURCES
    lib = capi.load_library()
    assert lib.gsttaco_style_affinities is not None and lib.gsttaco_style_map is not None


def test_export_gst_map_round_trips(tmp_path):
    y = S.blobs_run(0)[0][:5]
    wavs, tags = ["a/b c.wav", "d.wav", "e.wav", "f.wav", "g.wav"], ["AWB", "BDL", "AWB", "SLT", 7]
    path = str(tmp_path / "GST" / "L.GST.MAP.TXT")
    export.export_gst_map(path, wavs, tags, y)
    lines = open(path).read().split("\n")
    assert lines[0].split("\t") == ["Wav", "Tag", "TSNE_x", "TSNE_y"] and len(lines) == 6
    rows = [line.split("\t") for line in lines[1:]]
    assert [r[0] for r in rows] == wavs and [r[1] for r in rows] == [str(t) for t in tags]
    assert np.array_equal(np.array([[float(r[2]), float(r[3])] for r in rows]), y)
    gst_path = str(tmp_path / "GST" / "L.GST.TXT")                      # formatted as export_gst formats
    export.export_gst(gst_path, wavs, tags, y.astype(np.float64))
    assert [line.split("\t")[2:] for line in open(gst_path).read().split("\n")[1:]] == [r[2:] for r in rows]


def test_plot_gst_map_writes_the_figure(tmp_path):
    pytest.importorskip("matplotlib")
    path = str(tmp_path / "L.GST.PNG")
    export.plot_gst_map(path, [str(t) for t in S.BLOBS_LABELS], S.blobs_run(0)[0])
    assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"


def test_the_default_init_and_the_signatures():
    from gst_tacotron_amd import model
    for n, seed in ((120, 0), (7, 3)):
        want = np.random.default_rng(seed).standard_normal((n, 2)) * 1e-4
        assert np.array_equal(model.style_map_init(n, seed), want) and np.array_equal(S.default_init(n, seed), want)
    sig = inspect.signature(model.GST_Tacotron.Inference_GST)
    assert list(sig.parameters) == ["self", "wav_List", "tag_List", "label", "style_map"] and sig.parameters["style_map"].default is False
    sm = inspect.signature(model.GST_Tacotron.Style_Map).parameters
    assert list(sm) == ["self", "embeddings", "affinities", "perplexity", "iters", "seed", "init", "state", "exaggeration", "stop_lying_iter",
                        "mom_switch_iter", "momentum", "final_momentum", "eta"]
    assert {k: sm[k].default for k in S.DEFAULTS} == S.DEFAULTS and sm["perplexity"].default == 5.0 and sm["iters"].default == 1000
    assert inspect.signature(model.GST_Tacotron.Style_Affinities).parameters["perplexity"].default == 5.0
