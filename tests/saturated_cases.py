"""Cases in the regime a trained model lives in -- gates pinned at 0 and 1, a one-hot alignment that walks, p rounding to 1.0f, tanh
arguments in the tens -- for tests/test_gpu_saturated.py (on the GPU) and tests/test_saturated_cases.py (on the CPU: that every
case is in that regime, is well conditioned in float32, and that a wrong kernel form would be seen).

``weights.synthetic_weights`` gives Glorot kernels and biases of sigma 0.05: the largest decoder gate pre-activation is 1.6 and no
attention probability leaves (1e-4, 1 - 1e-4).  ``trained_like`` moves a synthetic weight dict into the other regime through the
LSTM biases and the attention's scales, NOT through one global gain: a gain makes the recurrences chaotic (float32 and float64 of
the oracle then part by 3.2 in the mel at gain 6 after 6 steps), which says nothing about a kernel.

Every case is ADMITTED by the oracle alone before a kernel is compared on it (``admit``): 8 x its float32 floor (max |oracle float32 -
oracle float64|) is at most ADMIT = 2e-4, a fifth of the 1e-3 north-star bar, for every compared output, and the regime conditions of
its recipe hold (``CONDITIONS``).  On the GPU the tolerance of an output is ``tolerance(floor)`` = max(TOL, 8 x floor): the kernels
differ from NumPy float32 in summation order and one-ulp hardware exp / rcp; at Glorot scale the recorded mel error is 3.8e-6 over a
floor of 1.1e-6, a ratio of 3.5, and 8 is twice that.  The floor comes from the oracle, never from a kernel.

BMA IS SPECIAL.  Where 1 - p falls between about 1e-10 and 1e-6 the reference's own safe-cumprod (Steps.py:183-199) is ill
conditioned: float32 rounds 1 - p to 0 and clips it to ``tiny``, float64 does not, and the 1e-10 clip of the cumulative product then
amplifies the difference (score_bias 25 over 10 steps: the two oracles disagree by 3.8e-2 in the alignment).  That is Steps.py, not a
kernel, so BMA is compared over the first 3 steps of an admitted case only, and ``admit`` rejects the score_bias-25 case.
"""
import collections
import functools

import numpy as np

from gst_tacotron_amd import synthetic, weights
from oracle import oracle_np

TOL = 5e-5              # tests/test_gpu_parity.py's: the project's fp32 bar against the float64 oracle
ADMIT = 2e-4            # 8 x floor must stay below a fifth of the north-star bar
FLOOR_FACTOR = 8.0
WEIGHT_SEED, BIAS_SEED, INPUT_SEED = 5, 9, 1

Recipe = collections.namedtuple("Recipe", "att sigma_b g_k g_v score_bias g_m g_q")
RECIPES = {
    #                     att        sigma_b g_k   g_v   score_bias g_m   g_q
    "glorot":     Recipe("SMA",       None, None, None, None,      None, None),      # the suite's own regime: the baseline
    "sma_sharp":  Recipe("SMA",       10.0, 2.0,  10.0, 10.0,      4.0,  4.0),
    "sma_wide":   Recipe("SMA",       10.0, 2.0,  10.0, 10.0,      4.0,  24.0),      # |q + pm| past 44.4, where exp(2x) leaves float32
    "sma_long":   Recipe("SMA",       10.0, 2.0,  10.0, 10.0,      1.0,  1.0),
    "lsa_sharp":  Recipe("LSA/32/31", 10.0, 2.0,  None, None,      8.0,  8.0),
    "lsa_smooth": Recipe("LSA/32/31/s", 10.0, 2.0, None, None,     8.0,  8.0),
    "bma":        Recipe("BMA",       10.0, 2.0,  10.0, 10.0,      2.0,  1.0),      # (g_m 2, see the BMA case below)
    "bma_bias25": Recipe("BMA",       10.0, 2.0,  10.0, 25.0,      1.0,  1.0),      # the ill-conditioned one: must be REJECTED
    "encoder":    Recipe("SMA",       10.0, None, None, None,      None, None),      # biases only: encoder / vocoder BiLSTM, highway
}

Spec = collections.namedtuple("Spec", "recipe B Tv steps lengths mixed wseed iseed", defaults=(WEIGHT_SEED, INPUT_SEED))
CASES = {
    #                        recipe        B   Tv   steps lengths            mixed
    "glorot":          Spec("glorot",      5,  40,  8,    None,              False),
    "sma_sharp":       Spec("sma_sharp",   5,  40,  8,    None,              False),   # the one-group persistent kernel
    "sma_sharp_group": Spec("sma_sharp",   40, 24,  6,    None,              False),   # the group kernel: two groups of rows
    "sma_wide":        Spec("sma_wide",    5,  40,  8,    None,              False),
    "sma_long_masked": Spec("sma_long",    4,  140, 8,    (140, 1, 57, 101), False),   # > 128 tokens, ragged, one utterance of ONE token
    # BMA scores are row-wide at g_m 1 (the tiled style embedding and the query dominate the 40 positions' differences): a row is either
    # all p ~ 1 or all p ~ 0, and an all-0 row loses its alignment mass at once.  No weights seed of 5..64 and no input seed of 1..2300 gave
    # five rows that keep their mass (row sums >= 0.9) AND 5 % of p below 1e-4; g_m 2 with weights seed 62 and input seed 3 does.
    "bma":             Spec("bma",         5,  40,  3,    None,              False, 62, 3),
    "lsa_sharp":       Spec("lsa_sharp",   5,  40,  8,    None,              False),
    "lsa_smooth":      Spec("lsa_smooth",  5,  40,  8,    None,              False),
    # (the issue's own setting of the rejected control -- g_m 1, seeds 5 / 9 / 1: it differs from "bma" in more than score_bias and steps)
    "bma_bias25":      Spec("bma_bias25",  5,  40,  10,   None,              False),
    "sma_sharp_mixed": Spec("sma_sharp",   40, 40,  8,    None,              True),    # bf16: persistent against launch path only
}
ADMITTED = ["sma_sharp", "sma_sharp_group", "sma_wide", "sma_long_masked", "bma", "lsa_sharp", "lsa_smooth"]

# regime conditions (share name, at least), each at roughly half of what the float64 oracle shows on the recipe at 3 x 40 tokens
_GATES = (("z_gt_8", 0.2), ("z_gt_16", 0.05))
_MONO = (("p_lt_1e-4", 0.05), ("p_gt_1-1e-4", 0.05), ("one_minus_p_lt_6e-8", 0.01))
CONDITIONS = {
    "sma_sharp": _GATES + _MONO + (("row0_advance", 4),),
    "sma_sharp_group": _GATES + _MONO,            # (6 steps: the walk is the 8-step case's business)
    "sma_wide": _GATES + _MONO + (("max_tanh_arg", 50.0),),
    "sma_long_masked": _GATES + _MONO,
    "bma": _GATES + _MONO + (("min_row_sum", 0.9),),
    "bma_bias25": _GATES + _MONO,
    "lsa_sharp": _GATES + (("max_align", 0.5),),
    "lsa_smooth": _GATES,                         # (sigmoid / sum cannot be one-hot: the softmax case carries the alignment condition)
}


def tolerance(floor):
    return max(TOL, FLOOR_FACTOR * floor)


# ---------------------------------------------------------------------------------------------------- weights
def _is_lstm_bias(name):
    return name.endswith(".bias") and (name.startswith("decoder.lstm") or name.startswith("encoder.bilstm.")
                                       or name.startswith("vocoder.bilstm."))


def _is_highway_bias(name):
    return name.startswith("vocoder.highway") and (name.endswith(".relu.bias") or name.endswith(".sigmoid.bias"))


def trained_like(w, recipe, rng):
    """A copy of the synthetic weight dict ``w`` moved to where a trained model saturates: N(0, sigma_b) on every LSTM bias (decoder,
    encoder BiLSTM, vocoder BiLSTM) and on the vocoder's highway biases, the decoder LSTM kernels and recurrent kernels times g_k,
    the attention's v times g_v, its score bias SET, its value / query kernels times g_m / g_q; LSA: N(0, 3) on the attention bias.
    A field that is None leaves its tensors alone."""
    out = {k: np.array(v, dtype=np.float32, copy=True) for k, v in w.items()}

    def scale(name, g):
        out[name] = (out[name] * np.float32(g)).astype(np.float32)

    for name in out:                                                        # (manifest order: the draws are reproducible)
        if recipe.sigma_b is not None and (_is_lstm_bias(name) or _is_highway_bias(name)):
            out[name] = (out[name] + rng.normal(0.0, recipe.sigma_b, out[name].shape)).astype(np.float32)
        if recipe.g_k is not None and name.startswith("decoder.lstm") and name.endswith("kernel"):
            scale(name, recipe.g_k)
    if recipe.g_v is not None and "decoder.attention.v" in out:
        scale("decoder.attention.v", recipe.g_v)
    if recipe.score_bias is not None and "decoder.attention.score_bias" in out:
        out["decoder.attention.score_bias"] = np.asarray(recipe.score_bias, np.float32)
    if recipe.g_m is not None:
        scale("decoder.attention.value.kernel", recipe.g_m)
    if recipe.g_q is not None:
        scale("decoder.attention.query.kernel", recipe.g_q)
    if recipe.sigma_b is not None and "decoder.attention.bias" in out:
        out["decoder.attention.bias"] = (out["decoder.attention.bias"] + rng.normal(0.0, 3.0, out["decoder.attention.bias"].shape)).astype(np.float32)
    return out


def full_hp(att="SMA", mixed=False):
    """synthetic.config_hp("cfg2") with the attention ``att``: "SMA", "BMA" or "LSA/filters/kernel[/s]" (s: smoothing)."""
    hp = synthetic.config_hp("cfg2")
    dec = hp["Tacotron2"]["Decoder"]
    if att.startswith("LSA"):
        p = att.split("/")
        dec["Attention"] = {"Type": "LSA", "Size": 128, "Conv": {"Filters": int(p[1]), "Kernel_Size": int(p[2])}, "Smoothing": len(p) > 3}
    else:
        dec["Attention"]["Type"] = att
    hp["Use_Mixed_Precision"] = bool(mixed)
    return hp


@functools.lru_cache(maxsize=None)
def recipe_weights(recipe_name, mixed=False, identity=False, wseed=WEIGHT_SEED):
    """(hp, weights) of a recipe: synthetic weights of seed ``wseed`` through ``trained_like`` with a generator of BIAS_SEED."""
    r = RECIPES[recipe_name]
    hp = full_hp(r.att, mixed)
    w = weights.synthetic_weights(hp, seed=wseed)
    return hp, (w if identity else trained_like(w, r, np.random.default_rng(BIAS_SEED)))


# ---------------------------------------------------------------------------------------------------- the traced decoder
def oracle_score(w, q, pm):
    """Steps.py:152 as oracle_np.attention_step states it."""
    return (w["decoder.attention.v"] * np.tanh(q[:, None, :] + pm)).sum(-1) + w["decoder.attention.score_bias"]


def hoisted_score(w, q, pm):
    """THE CONTROL, a form no kernel may take: tanh(q + m) = (E_q E_m - 1) / (E_q E_m + 1) with E_q = exp(2 q) per step and
    E_m = exp(2 m) hoisted out of the loop.  Exact in exact arithmetic; in float32 E overflows past |x| = 44.4 and inf / inf is NaN."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(2 * q)[:, None, :] * np.exp(2 * pm)
        return (w["decoder.attention.v"] * ((e - 1) / (e + 1))).sum(-1) + w["decoder.attention.score_bias"]


def traced_decoder(hp, w, memory, dt, prenet_masks, attn_noise, steps, token_lengths=None, score_fn=oracle_score):
    """oracle_np.decoder (fp32 / fp64 form, no mixed emulation) composed from the oracle's own step functions, with the attention step
    opened up so the gate pre-activations, the attention probabilities and the tanh arguments can be read and the score pass replaced
    (``score_fn``).  tests/test_saturated_cases.py holds it bitwise to oracle_np.decoder.  Returns pre, stops, aligns, trace."""
    mel, r = int(hp["Sound"]["Mel_Dim"]), int(hp["Step_Reduction"])
    att = hp["Tacotron2"]["Decoder"]["Attention"]
    B, Tv, _ = memory.shape
    pm = oracle_np.process_memory(w, memory)
    sizes = hp["Tacotron2"]["Decoder"]["RNN"]["Size"]
    hs = [np.zeros((B, s), dt) for s in sizes]
    cs = [np.zeros((B, s), dt) for s in sizes]
    frame = np.zeros((B, mel), dt)
    is_lsa = att["Type"] == "LSA"
    align = np.zeros((B, Tv), dt)
    if not is_lsa:
        align[:, 0] = 1.0
    lsa_state = np.zeros((B, Tv), dt)
    pre = np.zeros((B, steps * r, mel), dt)
    stops = np.zeros((B, steps), dt)
    aligns = np.zeros((B, steps, Tv), dt)
    valid = np.ones((B, Tv), bool) if token_lengths is None else np.arange(Tv)[None, :] < np.asarray(token_lengths)[:, None]
    sn = att.get("Sigmoid_Noise", 2.0 if att["Type"] == "SMA" else 0.0)
    trace = {"z": [], "p": [], "max_tanh_arg": 0.0}
    for t in range(steps):
        p = oracle_np.prenet(hp, w, frame, np.asarray(prenet_masks[t], dt))
        q = p @ w["decoder.attention.query.kernel"] + w["decoder.attention.query.bias"]
        if is_lsa:
            lsa_in = lsa_state * valid if token_lengths is not None else lsa_state
            ctx, align, lsa_state = oracle_np.lsa_step(hp, w, p, pm, lsa_in, token_lengths)
            arg = np.abs(q[:, None, :] + pm)
        else:
            score = score_fn(w, q, pm)
            if sn > 0.0:
                score = score + score.dtype.type(sn) * np.asarray(attn_noise[t], dt)
            align = oracle_np.monotonic_alignment(att["Type"], score, align, token_lengths)
            ctx = np.einsum("bt,bta->ba", align, pm)
            with np.errstate(over="ignore", invalid="ignore"):
                trace["p"].append(oracle_np.sigmoid(score)[valid])
            arg = np.abs(q[:, None, :] + pm)
        trace["max_tanh_arg"] = max(trace["max_tanh_arg"], float(arg[valid].max()))
        x = np.concatenate([p, ctx], -1)
        for i in range(len(sizes)):
            k, u, b = w[f"decoder.lstm{i}.kernel"], w[f"decoder.lstm{i}.recurrent_kernel"], w[f"decoder.lstm{i}.bias"]
            trace["z"].append(x @ k + hs[i] @ u + b)
            hs[i], cs[i] = oracle_np.lstm_cell(x, hs[i], cs[i], k, u, b)
            x = hs[i]
        y = np.concatenate([x, ctx], -1) @ w["decoder.projection.kernel"] + w["decoder.projection.bias"]
        pre[:, t * r:(t + 1) * r] = y[:, :mel * r].reshape(B, r, mel)
        stops[:, t] = y[:, mel * r]
        aligns[:, t] = align
        frame = pre[:, (t + 1) * r - 1]
    return pre, stops, aligns, trace


# ---------------------------------------------------------------------------------------------------- cases
Case = collections.namedtuple("Case", "name spec hp w tokens token_lengths mels mel_lengths masks noise")


def make_case(name, identity=False):
    """Weights and seeded inputs of CASES[name].  ``identity``: the same inputs on the untouched synthetic weights (what the case
    would be if ``trained_like`` did nothing)."""
    spec = CASES[name]
    hp, w = recipe_weights(spec.recipe, spec.mixed, identity, spec.wseed)
    rng = np.random.default_rng(spec.iseed)
    tokens, _ = synthetic.make_tokens(rng, spec.B, spec.Tv)                 # (full rows; ``lengths`` masks them: a length of 1 exists)
    mels, ml = synthetic.make_ref_mels(rng, spec.B, 12)
    masks, noise = synthetic.make_randomness(rng, spec.steps, spec.B, spec.Tv, hp["Tacotron2"]["Decoder"]["Prenet"]["Size"])
    tl = None if spec.lengths is None else np.asarray(spec.lengths, np.int32)
    return Case(name, spec, hp, w, tokens, tl, mels, ml, masks, noise)


def _err(a, b):
    with np.errstate(invalid="ignore"):
        e = np.abs(np.asarray(a, np.float64) - b)
    return float(e.max()) if np.isfinite(e).all() else float("inf")


def _shares(case, dec64, enc32):
    pre, stops, aligns, tr = dec64
    z = np.abs(np.concatenate([a.ravel() for a in tr["z"]]))
    s = {"z_gt_8": float((z > 8).mean()), "z_gt_16": float((z > 16).mean()), "max_z": float(z.max()),
         "max_tanh_arg": tr["max_tanh_arg"], "max_align": float(aligns.max()),
         "enc_h_eq_1": float((np.abs(enc32) == np.float32(1.0)).mean()),
         "row_sums": aligns.sum(-1), "argmax_path": aligns.argmax(-1)}
    s["min_row_sum"] = float(s["row_sums"].min())
    s["row0_advance"] = int(s["argmax_path"][0].max() - s["argmax_path"][0][0])
    if tr["p"]:
        p = np.concatenate(tr["p"])
        s.update({"p_lt_1e-4": float((p < 1e-4).mean()), "p_gt_1-1e-4": float((p > 1 - 1e-4).mean()),
                  "one_minus_p_lt_6e-8": float((1 - p < 6e-8).mean())})
    return s


def measure(case, end_to_end=False):
    """The oracle on a case in float64 and in float32.  Returns a dict:
    ``f32``     the float32 decoder's pre_mel, stop, align on the float64 memory cast to float32
    ``ref``     float64 outputs: encoder, gst, pre_mel, stop, align from the decoder alone on the float64 memory (what
                ``GST_Tacotron.decode`` is fed), and with ``end_to_end`` mel, spectrogram
    ``floor``   max |float32 - float64| per output: encoder; pre_mel, stop, align of the float32 decoder on the float64 memory cast to
                float32; with ``end_to_end`` e2e_mel, e2e_stop, e2e_align, e2e_spectrogram of the whole float32 pipeline
    ``shares``  the regime: shares of decoder gate |z| > 8 / > 16, of p < 1e-4, p > 1 - 1e-4, 1 - p < 6e-8 (float64 p over the valid
                positions), of encoder states that are exactly +-1.0f in float32, max |q + pm|, alignment row sums and argmax path."""
    c = case
    tl = c.token_lengths
    out = {}
    with np.errstate(over="ignore"):        # (exp(-x) of a score of -100 overflows to inf in float32: sigmoid = 0, as it should be)
        for dt in (np.float64, np.float32):
            w = oracle_np.cast_weights(c.w, dt)
            enc = oracle_np.encoder(c.hp, w, c.tokens, dt, tl)
            gst = oracle_np.style_token_layer(c.hp, w, c.mels, c.mel_lengths, dt)
            out[dt] = {"w": w, "enc": enc, "gst": gst}
        e64 = out[np.float64]
        mem64 = oracle_np.gst_concat(e64["enc"], e64["gst"])
        dec64 = traced_decoder(c.hp, e64["w"], mem64, np.float64, c.masks, c.noise, c.spec.steps, tl)
        dec32 = traced_decoder(c.hp, out[np.float32]["w"], mem64.astype(np.float32), np.float32, c.masks, c.noise, c.spec.steps, tl)
        ref = {"encoder": e64["enc"], "gst": e64["gst"], "pre_mel": dec64[0], "stop": dec64[1], "align": dec64[2]}
        floor = {"encoder": _err(out[np.float32]["enc"], e64["enc"]),
                 "pre_mel": _err(dec32[0], dec64[0]), "stop": _err(dec32[1], dec64[1]), "align": _err(dec32[2], dec64[2])}
        if end_to_end:
            e32 = out[np.float32]
            full32 = traced_decoder(c.hp, e32["w"], oracle_np.gst_concat(e32["enc"], e32["gst"]), np.float32, c.masks, c.noise, c.spec.steps, tl)
            mel64 = oracle_np.postnet(c.hp, e64["w"], dec64[0], np.float64)
            mel32 = oracle_np.postnet(c.hp, e32["w"], full32[0], np.float32)
            ref["mel"], ref["spectrogram"] = mel64, oracle_np.vocoder_taco1(c.hp, e64["w"], mel64, np.float64)
            floor.update({"e2e_mel": _err(mel32, mel64), "e2e_stop": _err(full32[1], dec64[1]), "e2e_align": _err(full32[2], dec64[2]),
                          "e2e_spectrogram": _err(oracle_np.vocoder_taco1(c.hp, e32["w"], mel32, np.float32), ref["spectrogram"])})
    f32 = {"pre_mel": dec32[0], "stop": dec32[1], "align": dec32[2]}
    return {"ref": ref, "f32": f32, "floor": floor, "shares": _shares(c, dec64, out[np.float32]["enc"])}


END_TO_END = ("sma_sharp",)         # the cases whose measurement also holds the whole pipeline's floors (postnet, vocoder)


@functools.lru_cache(maxsize=None)
def measured(name):
    """``measure(make_case(name))`` once per process: the reference is shared among the tests that need it and left unchanged."""
    c = make_case(name)
    return c, measure(c, name in END_TO_END)


def admit(m, conditions, outputs=None):
    """The reasons for which a measured case is NOT admitted ([] = admitted): an output whose 8 x floor exceeds ADMIT, a regime
    condition (share name, at least) that does not hold.  The oracle alone decides; no kernel is involved."""
    why = []
    for k, f in m["floor"].items():
        if (outputs is None or k in outputs) and not FLOOR_FACTOR * f <= ADMIT:
            why.append("floor of %s: 8 x %.3g > %.3g" % (k, f, ADMIT))
    for k, least in conditions:
        if not m["shares"][k] >= least:
            why.append("regime %s: %.3g < %.3g" % (k, m["shares"][k], least))
    return why


def describe(name, m):
    s = m["shares"]
    keys = [k for k in ("z_gt_8", "z_gt_16", "p_lt_1e-4", "p_gt_1-1e-4", "one_minus_p_lt_6e-8", "max_tanh_arg", "max_align", "min_row_sum",
                        "row0_advance", "enc_h_eq_1") if k in s]
    return "%s floors %s shares %s" % (name, {k: float("%.3g" % v) for k, v in m["floor"].items()}, {k: float("%.3g" % s[k]) for k in keys})


# ---------------------------------------------------------------------------------------------------- encoder / vocoder
ENCODER_SHAPES = [(17, 33), (33, 20)]


def encoder_lengths(B, Tv):
    """Ragged lengths that include 1, 2 and the full length."""
    tl = np.random.default_rng(B * 100 + Tv).integers(1, Tv + 1, B).astype(np.int32)
    tl[0], tl[1], tl[2] = 1, 2, Tv
    return tl


@functools.lru_cache(maxsize=None)
def encoder_case(B, Tv, masked):
    """(hp, w, tokens, lengths or None, float64 encodings, float32 floor, share of float32 states that are exactly +-1.0f, share below 1e-6)
    of the encoder recipe."""
    hp, w = recipe_weights("encoder")
    tokens, _ = synthetic.make_tokens(np.random.default_rng(INPUT_SEED + B), B, Tv)
    tl = encoder_lengths(B, Tv) if masked else None
    ref = oracle_np.encoder(hp, oracle_np.cast_weights(w, np.float64), tokens, np.float64, tl)
    f32 = oracle_np.encoder(hp, oracle_np.cast_weights(w, np.float32), tokens, np.float32, tl)
    live = np.ones(f32.shape[:2], bool) if tl is None else np.arange(Tv)[None, :] < tl[:, None]
    return hp, w, tokens, tl, ref, _err(f32, ref), float((np.abs(f32[live]) == np.float32(1.0)).mean()), float((np.abs(f32[live]) < 1e-6).mean())


VOCODER_SHAPE = (3, 21)


def _traced_vocoder(hp, w, mel):
    """oracle_np.vocoder_taco1 in float64 with the highway gates' pre-activations t and the BiLSTM's gate pre-activations z recorded
    (the oracle's own ``highway`` and ``lstm_cell`` wrapped for the duration of the call)."""
    t, z = [], []
    highway, cell = oracle_np.highway, oracle_np.lstm_cell

    def traced_highway(y, w_relu, b_relu, w_sig, b_sig):
        t.append(np.abs(y @ w_sig + b_sig).ravel())
        return highway(y, w_relu, b_relu, w_sig, b_sig)

    def traced_cell(x, h, c, kernel, rec, bias):
        z.append(np.abs(x @ kernel + h @ rec + bias).ravel())
        return cell(x, h, c, kernel, rec, bias)

    oracle_np.highway, oracle_np.lstm_cell = traced_highway, traced_cell
    try:
        ref = oracle_np.vocoder_taco1(hp, w, mel, np.float64)
    finally:
        oracle_np.highway, oracle_np.lstm_cell = highway, cell
    return ref, np.concatenate(t), np.concatenate(z)


VOCODER_CONDITIONS = (("t_gt_8", 0.2), ("z_gt_8", 0.2), ("z_gt_16", 0.05))     # (about half of what the float64 oracle shows)


@functools.lru_cache(maxsize=None)
def vocoder_case(identity=False):
    """(hp, w, mel, float64 spectrogram, float32 floor, shares) of the encoder / vocoder recipe; the shares are the float64 oracle's:
    highway gate pre-activations |t| > 8, vocoder BiLSTM gate pre-activations |z| > 8 and > 16."""
    hp, w = recipe_weights("encoder", identity=identity)
    B, T = VOCODER_SHAPE
    mel = np.clip(np.random.default_rng(INPUT_SEED).normal(0, 1.5, (B, T, 80)), -4, 4).astype(np.float32)
    ref, t, z = _traced_vocoder(hp, oracle_np.cast_weights(w, np.float64), mel.astype(np.float64))
    f32 = oracle_np.vocoder_taco1(hp, oracle_np.cast_weights(w, np.float32), mel, np.float32)
    shares = {"t_gt_8": float((t > 8).mean()), "z_gt_8": float((z > 8).mean()), "z_gt_16": float((z > 16).mean())}
    return hp, w, mel, ref, _err(f32, ref), shares
