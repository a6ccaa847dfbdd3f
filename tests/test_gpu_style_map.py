"""GPU tests of the style map: gsttaco_style_affinities and gsttaco_style_map (csrc/tsne.hip) against the float64 restatement of
tests/style_map_cases.py -- beta and the search's round counts exactly, p, y, velocity and gains to RTOL --, the full 1000-step run by
what it must achieve, every refusal straight through the C ABI, and Inference_GST(style_map=...) end to end."""
import ctypes
import os

import numpy as np
import pytest

import style_map_cases as S
from gst_tacotron_amd import synthetic

pytestmark = pytest.mark.gpu

_MODELS = {}
TINY = 2.0 ** -1022             # below the smallest normal a double carries no relative accuracy


@pytest.fixture(scope="module", autouse=True)
def _close_the_contexts():
    """The context of ``_model`` lives for this module only (the persistent decode launch of later files needs to be the process's one
    live context)."""
    yield
    for m in _MODELS.values():
        m.ctx.close()
    _MODELS.clear()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _np(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _model():
    """One context without weights (neither entry needs any), kept for the module."""
    from gst_tacotron_amd.model import GST_Tacotron
    if "m" not in _MODELS:
        _MODELS["m"] = GST_Tacotron(hyper_parameters=synthetic.tiny_hp(), max_batch=2, max_tokens=8, max_ref_frames=4, max_wav_seconds=0.0)
    return _MODELS["m"]


def _state(c, m):
    import torch
    y, v, g = (torch.from_numpy(np.array(a)).to(m.device) for a in c.state)
    return dict(y=y, velocity=v, gains=g, iter=c.first_iter)


def _same(a, b, keys=("y", "velocity", "gains", "kl")):
    return all(np.array_equal(*_np(a[k], b[k])) for k in keys)


# ---------------------------------------------------------------------------------------------------- 1. the affinities, case by case
@pytest.mark.parametrize("name", S.AFFINITY_NAMES)
def test_affinities_equal_the_float64_restatement(name):
    import torch
    c = S.AFFINITY_CASES[name]
    want = S.affinity_reference(name)
    m = _model()
    x = torch.from_numpy(np.array(c.wide)).to(m.device)[:, :c.D]            # ldx > D: a view, read where it lies
    assert x.stride(0) == c.ldx
    p, beta, rounds = _np(*m.Style_Affinities(x, c.perplexity))
    assert p.dtype == beta.dtype == np.float64 and rounds.dtype == np.int32 and p.shape == (c.N, c.N)
    assert np.array_equal(rounds, want["search_iters"]), (name, rounds, want["search_iters"])
    assert np.array_equal(beta, want["beta"]), name
    err = np.abs(p - want["p"])
    nz = want["p"] > TINY
    print(name, "rounds", rounds.min(), "..", rounds.max(), "largest relative error of p", float((err[nz] / want["p"][nz]).max()),
          "sum p - 1", p.sum() - 1)
    assert (err <= S.RTOL * np.abs(want["p"]) + TINY).all()
    assert np.array_equal(p, p.T) and (np.diag(p) == 0).all() and np.isfinite(p).all() and abs(p.sum() - 1) <= c.N * c.N * 2.0 ** -52
    again = _np(*m.Style_Affinities(x, c.perplexity))
    assert all(np.array_equal(a, g) for a, g in zip(again, (p, beta, rounds)))
    if c.ldx == c.D:                                                        # a host array gives the same bits
        host = _np(*m.Style_Affinities(np.array(c.x), c.perplexity))
        assert all(np.array_equal(a, g) for a, g in zip(host, (p, beta, rounds)))


# ---------------------------------------------------------------------------------------------------- 2. the descent, case by case
@pytest.mark.parametrize("name", S.DESCENT_NAMES)
def test_descent_equals_the_float64_restatement(name):
    import torch
    c = S.DESCENT_CASES[name]
    want = S.descent_case_reference(name)
    m = _model()
    p = torch.from_numpy(np.array(c.p)).to(m.device)
    start = _state(c, m)
    got = m.Style_Map(affinities=p, state=start, iters=c.iters, **c.schedule)
    y, v, g, kl = _np(got["y"], got["velocity"], got["gains"], got["kl"])
    assert got["iter"] == c.first_iter + c.iters and got["affinities"] is p and np.array_equal(_np(start["y"])[0], c.state[0])
    scale = float(np.abs(want["y"]).max())
    worst = max(float(np.abs(a - want[k]).max()) for a, k in ((y, "y"), (v, "velocity"), (g, "gains"))) / scale
    host_kl = S.kl_reference(c.p, y)
    print(name, "worst difference / max|y|", worst, "kl", float(kl), "relative to the host's", abs(float(kl) - host_kl) / host_kl)
    for a, k in ((y, "y"), (v, "velocity"), (g, "gains")):
        assert (np.abs(a - want[k]) <= S.RTOL * scale).all(), (name, k)
    assert abs(float(kl) - host_kl) <= S.RTOL * abs(host_kl)
    if c.kl_only:
        assert np.array_equal(y, c.state[0]) and np.array_equal(v, c.state[1]) and np.array_equal(g, c.state[2])
    assert _same(got, m.Style_Map(affinities=p, state=start, iters=c.iters, **c.schedule))
    if c.iters >= 2:                                                        # the state is (y, velocity, gains, iter) and nothing else
        half = m.Style_Map(affinities=p, state=start, iters=c.iters // 2, **c.schedule)
        assert half["iter"] == c.first_iter + c.iters // 2
        assert _same(got, m.Style_Map(state=half, iters=c.iters - c.iters // 2, **c.schedule))


# ---------------------------------------------------------------------------------------------------- 3. the full run
def test_the_full_run_separates_the_blobs():
    m = _model()
    x = np.array(S.AFFINITY_CASES["blobs120"].x)
    got = m.Style_Map(x)
    assert set(got) == {"y", "velocity", "gains", "iter", "kl", "affinities", "beta"} and got["iter"] == 1000
    y, v, g, kl, p, beta = _np(*(got[k] for k in ("y", "velocity", "gains", "kl", "affinities", "beta")))
    assert y.shape == (120, 2) and y.dtype == np.float64 and all(np.isfinite(a).all() for a in (y, v, g, kl, p, beta))
    assert np.array_equal(beta, S.affinity_reference("blobs120")["beta"])
    scale = np.abs(y).max()
    host_kl = S.kl_reference(p, y)
    print("blobs120 on the device: kl", float(kl), "purity", S.purity(y, S.BLOBS_LABELS), "column means / max|y|", np.abs(y.mean(axis=0)).max() / scale)
    assert np.abs(y.mean(axis=0)).max() <= 1e-12 * scale
    assert S.purity(y, S.BLOBS_LABELS) == 1.0
    assert float(kl) <= 1.25 * max(S.BLOBS_KL)
    assert abs(float(kl) - host_kl) <= S.RTOL * host_kl
    assert _same(got, m.Style_Map(x))
    first = m.Style_Map(x, iters=500)
    assert first["iter"] == 500 and _same(got, m.Style_Map(state=first, iters=500))
    other = _np(m.Style_Map(affinities=got["affinities"], seed=1)["y"])[0]  # a map depends on its seed
    assert not np.array_equal(other, y) and np.isfinite(other).all()
    given = _np(m.Style_Map(affinities=got["affinities"], init=S.default_init(120, 0))["y"])[0]
    assert np.array_equal(given, y)


def test_style_map_arguments():
    m = _model()
    x = np.array(S.AFFINITY_CASES["n7_d1"].x)
    p, _, _ = m.Style_Affinities(x, 2.0)
    with pytest.raises(ValueError, match="not both"):
        m.Style_Map(x, affinities=p)
    with pytest.raises(ValueError, match="embeddings or affinities"):
        m.Style_Map()
    with pytest.raises(ValueError, match="init or state"):
        m.Style_Map(state=m.Style_Map(affinities=p, iters=1), init=np.zeros((7, 2)))
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        m.Style_Map(affinities=p, init=np.zeros((6, 2)))


# ---------------------------------------------------------------------------------------------------- 4. the refusals
def test_style_affinities_refusals_write_nothing():
    import torch
    from gst_tacotron_amd import capi
    m = _model()
    lib, h = m.ctx.lib, m.ctx.handle
    N, D = 8, 4
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((N, D)).astype(np.float32)).to(m.device)
    p = torch.full((N + 1, N), float("nan"), dtype=torch.float64, device=m.device)
    beta = torch.full((N + 1,), float("nan"), dtype=torch.float64, device=m.device)
    rounds = torch.full((N + 1,), -7, dtype=torch.int32, device=m.device)

    def call(x_=x, N=N, D=D, ldx=D, perplexity=3.0, p_=p, beta_=beta, rounds_=rounds):
        return lib.gsttaco_style_affinities(h, _ptr(x_), N, D, ldx, ctypes.c_float(perplexity), _ptr(p_), _ptr(beta_), _ptr(rounds_), m._stream())
    assert call(x_=None) == -1 and "null" in m.last_message()
    assert call(p_=None) == -1 and call(beta_=None) == -1
    assert call(N=2, perplexity=1.5) == -1 and call(D=0) == -1 and call(ldx=D - 1) == -1
    for bad in (float("nan"), float("inf"), 1.0, 0.5, -3.0, float(N - 1), float(N)):
        assert call(perplexity=bad) == -1 and "perplexity" in m.last_message(), bad
    assert call(N=8193, perplexity=5.0) == -5 and "8192" in m.last_message()
    assert call(N=8193, perplexity=9000.0) == -1                            # an invalid argument is named before the capacity
    got = _np(p, beta, rounds)
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and (got[2] == -7).all()
    assert call(rounds_=None) == 0 and call() == 0                          # search_iters may be NULL; the call itself is fine
    got = _np(p, beta, rounds)
    assert np.isfinite(got[0][:N]).all() and np.isnan(got[0][N]).all() and np.isnan(got[1][N]) and got[2][N] == -7 and (got[2][:N] > 0).all()
    assert call(perplexity=float(np.nextafter(np.float32(N - 1), np.float32(0)))) == 0      # the open interval's inside
    with pytest.raises(capi.GstTacoError):
        m.Style_Affinities(np.zeros((8, 4), np.float32), perplexity=7.0)
    m.synchronize()


def test_style_map_refusals_write_nothing():
    import torch
    m = _model()
    lib, h = m.ctx.lib, m.ctx.handle
    N = 7
    p = m.Style_Affinities(np.array(S.AFFINITY_CASES["n7_d1"].x), 2.0)[0]
    y, v, g = (torch.full((N + 1, 2), float("nan"), dtype=torch.float64, device=m.device) for _ in range(3))
    for t, a in ((y, S.default_init(N, 0)), (v, np.zeros((N, 2))), (g, np.ones((N, 2)))):
        t[:N] = torch.from_numpy(a).to(m.device)
    before = _np(y, v, g)
    kl = torch.full((2,), float("nan"), dtype=torch.float64, device=m.device)
    cf = ctypes.c_float

    def call(p_=p, N=N, y_=y, v_=v, g_=g, first=0, iters=3, ex=12.0, stop=250, switch=250, mom=0.5, final=0.8, eta=200.0, kl_=kl):
        return lib.gsttaco_style_map(h, _ptr(p_), N, _ptr(y_), _ptr(v_), _ptr(g_), first, iters, cf(ex), stop, switch, cf(mom), cf(final),
                                     cf(eta), _ptr(kl_), m._stream())
    for k in ("p_", "y_", "v_", "g_"):
        assert call(**{k: None}) == -1 and "null" in m.last_message()
    assert call(N=2) == -1 and call(iters=-1) == -1 and call(first=-1) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(eta=bad) == -1 and call(ex=bad) == -1, bad
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert call(mom=bad) == -1 and call(final=bad) == -1 and "momentum" in m.last_message(), bad
    assert call(N=8193) == -5 and "8192" in m.last_message()
    after = _np(y, v, g, kl)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(after[:3], before)) and np.isnan(after[3]).all()
    assert call(iters=0, kl_=None) == 0                                      # nothing to do: nothing written
    after = _np(y, v, g)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(after, before))
    assert call(iters=0) == 0                                               # the KL alone
    yy, vv, gg, k = _np(y, v, g, kl)
    assert np.array_equal(yy, before[0], equal_nan=True) and np.isfinite(k[0]) and np.isnan(k[1])
    assert abs(k[0] - S.kl_reference(_np(p)[0], yy[:N])) <= S.RTOL * abs(k[0])
    assert call(kl_=None, mom=0.0, final=0.0) == 0                          # the limits themselves are accepted; kl may be NULL
    yy, vv, gg = _np(y, v, g)
    assert np.isfinite(yy[:N]).all() and np.isnan(yy[N]).all() and np.isnan(vv[N]).all() and np.isnan(gg[N]).all()
    assert not np.array_equal(yy[:N], before[0][:N])
    m.synchronize()


# ---------------------------------------------------------------------------------------------------- 5. end to end
def test_inference_gst_with_a_style_map(tmp_path):
    """synthetic.tiny_hp() with synthetic weights on 8 synthetic wavs: the flag changes neither the embeddings nor the table, the map is
    Style_Map of those embeddings, and the map's table (and, with matplotlib, its figure) lie beside the embedding table."""
    from gst_tacotron_amd import export, weights
    from gst_tacotron_amd.model import GST_Tacotron
    hp = synthetic.tiny_hp()
    hp["Inference_Path"] = str(tmp_path / "out")
    rng = np.random.default_rng(8)
    wavs, tags = [], []
    for i in range(8):
        n = 2000 + 150 * i
        sig = 0.3 * np.sin(np.arange(n) * 0.04 * (1 + i % 4)) + 0.02 * rng.standard_normal(n)
        wavs.append(str(tmp_path / ("ref%d.wav" % i)))
        export.write_wav(wavs[-1], sig, 16000)
        tags.append("AB"[i % 2])
    settings = dict(perplexity=2.0, iters=20)
    m = GST_Tacotron(hyper_parameters=hp, max_batch=8, max_tokens=8, max_ref_frames=256, max_wav_seconds=1.0)
    try:
        m.Restore(weights=weights.synthetic_weights(hp, seed=3))
        plain = m.Inference_GST(wavs, tags, label="P")
        gsts, smap = m.Inference_GST(wavs, tags, label="T", style_map=settings)
        assert gsts.device.type == "cuda" and np.array_equal(*_np(plain, gsts)) and tuple(gsts.shape) == (8, m.dims.gst_att)
        assert smap["iter"] == 20 and tuple(smap["y"].shape) == (8, 2)
        assert _same(smap, m.Style_Map(gsts, **settings)) and np.array_equal(*_np(smap["affinities"], m.Style_Map(gsts, **settings)["affinities"]))
        root = os.path.join(hp["Inference_Path"], "GST")
        assert open(os.path.join(root, "T.GST.TXT")).read() == open(os.path.join(root, "P.GST.TXT")).read()
        rows = [r.split("\t") for r in open(os.path.join(root, "T.GST.MAP.TXT")).read().split("\n")]
        assert rows[0] == ["Wav", "Tag", "TSNE_x", "TSNE_y"] and [r[0] for r in rows[1:]] == wavs and [r[1] for r in rows[1:]] == tags
        assert np.array_equal(np.array([[float(r[2]), float(r[3])] for r in rows[1:]]), _np(smap["y"])[0])
        assert not os.path.exists(os.path.join(root, "P.GST.MAP.TXT"))
        try:
            import matplotlib  # noqa: F401
            assert os.path.exists(os.path.join(root, "T.GST.PNG"))
        except ImportError:
            pass
        defaults = m.Inference_GST(wavs, style_map=True)                    # no tags: nothing written, TSNE.R's defaults
        assert defaults[1]["iter"] == 1000 and np.isfinite(_np(defaults[1]["y"])[0]).all() and sorted(os.listdir(root)) == sorted(
            ["P.GST.TXT", "T.GST.TXT", "T.GST.MAP.TXT"] + (["T.GST.PNG"] if os.path.exists(os.path.join(root, "T.GST.PNG")) else []))
    finally:
        m.ctx.close()


def test_without_the_gst_branch():
    from gst_tacotron_amd.model import GST_Tacotron
    hp = synthetic.tiny_hp(gst=False)
    m = GST_Tacotron(hyper_parameters=hp, max_batch=2, max_tokens=8, max_ref_frames=4, max_wav_seconds=0.0)
    try:
        with pytest.raises(NotImplementedError, match="GST is not used"):
            m.Inference_GST([np.zeros(2000, np.float32)], style_map=True)
        y = m.Style_Map(np.array(S.AFFINITY_CASES["n7_d1"].x), perplexity=2.0, iters=2)["y"]       # the map itself needs no GST branch
        assert np.isfinite(_np(y)[0]).all()
    finally:
        m.ctx.close()
