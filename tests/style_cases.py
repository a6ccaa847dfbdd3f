"""Float64 restatements and shared cases of the style-control tests: tests/test_gpu_style.py runs them on the GPU,
tests/test_style_cases.py checks on the CPU that they are well conditioned and can see what they are meant to see.

Notation (include/gsttaco.h): H heads, N style tokens, A = Style_Token.Attention.Size, dh = A / H,
V = tanh(tokens).Wv + bv [N, A].  The reference's layer (Layers.py:172-214; oracle_np.style_token_layer) is

    q        = ref.Wq + bq                                               [B, A]
    p[b,h,:] = softmax_n(q[b, h-slice] . V[:, h-slice]^T)                [B, H, N]
    gst      = LayerNorm(concat_h(p[b,h,:] . V[:, h-slice]) + q)

``export`` restates (p, q), ``compose`` the last line for GIVEN weights, both from oracle_np's public functions.  Shapes and
weights are gst_cases's.
"""
import functools

import numpy as np

import gst_cases as G
from oracle import oracle_np

# the five cases of the compose tests: cfg2 at G.SMALL, and four accepted size sets of the grid (16 / 256 / 32 / 128 wide, 4 / 8 / 1 / 4
# heads, 6 / 33 / 1 / 10 tokens)
GRID_NAMES = ["u16_tiny", "u64_dense64_att256_heads8_tok33", "u128_heads1_tok1", "u256_mel80_full_filters_tok10"]
CASES = ["cfg2"] + GRID_NAMES
# the export tests' sharper attention: the synthetic weights give nearly uniform p (the largest weight of 16 tokens is 0.12), which
# a p with its heads swapped would match within the tolerance.  The query kernel scaled by SHARPEN in a copy spreads the scores.
SHARPEN = 8.0


def _frozen(a):
    a = np.array(a, order="C")
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def sharp_weights():
    hp, w = G.cfg2_weights()
    w = dict(w)
    w["gst.mha.query.kernel"] = _frozen(w["gst.mha.query.kernel"] * np.float32(SHARPEN))
    return hp, w


def case(name):
    """(hp, float32 weights, Shape, mel bins) of a compose case, or of "cfg2_short" / "sharp_short" (G.SHORT: the export tests)."""
    if name == "cfg2":
        return G.cfg2_weights() + (G.SMALL, 80)
    if name == "cfg2_short":
        return G.cfg2_weights() + (G.SHORT, 80)
    if name == "sharp_short":
        return sharp_weights() + (G.SHORT, 80)
    c = G.GRID_BY_NAME[name]
    return c.hp, G.grid_weights(name), c.shape, c.mel


def reference(name):
    """The float64 style embeddings gst_cases already holds for a compose case."""
    return G.reference(G.SMALL) if name == "cfg2" else G.grid_reference(name)


def dims(hp):
    st = hp["GST"]["Style_Token"]
    return int(st["Attention"]["Head"]), int(st["Size"]), int(st["Attention"]["Size"])


def value_table(w):
    """V [N, A] in the dtype of ``w`` (GST.py:100-101, Layers.py:175)."""
    return np.tanh(w["gst.tokens"]) @ w["gst.mha.value.kernel"] + w["gst.mha.value.bias"]


def export(hp, w, mels, lens, dt=np.float64):
    """(p [B, H, N], q [B, A]) of a reference, evaluated in ``dt``."""
    w = oracle_np.cast_weights(w, dt)
    H, N, A = dims(hp)
    ref = oracle_np.reference_encoder(hp, w, np.asarray(mels, dt)[:, 1:], lens, dt)
    q = ref @ w["gst.mha.query.kernel"] + w["gst.mha.query.bias"]
    v = value_table(w)
    dh = A // H
    p = np.stack([oracle_np.softmax(q[:, h * dh:(h + 1) * dh] @ v[:, h * dh:(h + 1) * dh].T) for h in range(H)], axis=1)
    return p, q


def compose(hp, w, weights, query=None, dt=np.float64):
    """LayerNorm(concat_h(weights[b, h, :] . V[:, h-slice]) + query) in ``dt``; query None = 0."""
    w = oracle_np.cast_weights(w, dt)
    H, N, A = dims(hp)
    weights = np.asarray(weights, dt)
    assert weights.shape[1:] == (H, N)
    v = value_table(w)
    dh = A // H
    out = np.concatenate([weights[:, h] @ v[:, h * dh:(h + 1) * dh] for h in range(H)], axis=-1)
    if query is not None:
        out = out + np.asarray(query, dt)
    return oracle_np.layer_norm(out, w["gst.mha.ln.gamma"], w["gst.mha.ln.beta"])


@functools.lru_cache(maxsize=None)
def exported(name):
    """float64 (p, q) of a case's reference batch: computed once per process, read-only."""
    hp, w, shape, mel = case(name)
    p, q = export(hp, w, *G.inputs(shape, mel))
    return _frozen(p), _frozen(q)


@functools.lru_cache(maxsize=None)
def signed_weights(name):
    """Seeded float32 weights in [-0.5, 1) [B, H, N]: negative, above the softmax's range in sum, not normalised."""
    hp, _, shape, _ = case(name)
    H, N, _ = dims(hp)
    rng = np.random.default_rng(300 + sum(map(ord, name)))
    return _frozen(rng.uniform(-0.5, 1.0, (shape.B, H, N)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def signed_reference(name):
    hp, w, _, _ = case(name)
    return _frozen(compose(hp, w, signed_weights(name)))
