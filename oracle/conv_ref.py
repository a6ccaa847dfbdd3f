"""Float64 reference of the conv/GEMM dispatcher's contract (gst_tacotron_amd/csrc/kernels.h, ConvGemmArgs):

    out[(b,t), n] = act( scale[n] * sum_{tap,c} X[b, t + tap - pad_before, c] * w[tap*Cin + c, n] + shift[n] + rowbias[b,n] ) + res

with X the gathered input: row (b, s) is x[tokens[b,s]] (or x[b*T + s]), rows s outside [0, min(T, row_len[b])) read as zero, and
with pool2 a row is max(X[s], X[s+1]) where s+1 is still inside the length (padding never wins the max).  2-D mode: rows are
(b, ho, wo), T = Ho*Wo, tap = i*kw + j reads x[b][ho*stride + i - pad_h][wo*stride + j - pad_w][c] of an NHWC input.

Besides y it returns the magnitude m = |scale| * (|W| conv |X|) + |shift| + |rowbias|: the same sum on absolute values, the scale
of any rounding error a summation order can make.  bf16=True rounds both operands to bf16 (RNE) first, as the mixed-precision
kernels do on their way into LDS.
"""
import numpy as np

from oracle.oracle_np import bf16_round

ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2


def gather_rows(x, B, T, Cin, taps, pad_before, tokens=None, row_len=None, pool2=False):
    """The im2col operand as a list over taps of [B, T, Cin] float64 arrays (tap j: input frame t + j - pad_before)."""
    if tokens is not None and pool2:
        raise ValueError("tokens with pool2 is not a combination the dispatcher's kernels implement")
    x = np.asarray(x, dtype=np.float64)
    if tokens is not None:
        rows = x.reshape(-1, Cin)[np.asarray(tokens).reshape(B, T)]
    else:
        rows = x.reshape(B, T, Cin)
    lens = np.full(B, T) if row_len is None else np.minimum(T, np.asarray(row_len).reshape(B))
    valid = np.arange(T)[None, :] < lens[:, None]                   # [B, T]
    rows = np.where(valid[:, :, None], rows, 0.0)
    if pool2:
        nxt = np.concatenate([rows[:, 1:], np.zeros_like(rows[:, :1])], 1)
        nxt_ok = np.concatenate([valid[:, 1:], np.zeros_like(valid[:, :1])], 1)
        rows = np.where(nxt_ok[:, :, None], np.maximum(rows, nxt), rows)
    out = []
    for j in range(taps):
        d = j - pad_before
        g = np.zeros_like(rows)
        lo, hi = max(0, -d), min(T, T - d)
        if hi > lo:
            g[:, lo:hi] = rows[:, lo + d:hi + d]
        out.append(g)
    return out


def gather_rows_2d(x, B, H, W, Cin, kh, kw, stride, pad_h, pad_w, Ho, Wo, xb=None):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    xb = H * W * Cin if xb is None else xb
    xs = np.stack([x[b * xb:b * xb + H * W * Cin].reshape(H, W, Cin) for b in range(B)])
    out = []
    for i in range(kh):
        for j in range(kw):
            g = np.zeros((B, Ho, Wo, Cin))
            for ho in range(Ho):
                hi = ho * stride + i - pad_h
                if not 0 <= hi < H:
                    continue
                for wo in range(Wo):
                    wi = wo * stride + j - pad_w
                    if 0 <= wi < W:
                        g[:, ho, wo] = xs[:, hi, wi]
            out.append(g.reshape(B, Ho * Wo, Cin))
    return out


def conv_gemm_ref(x, w, B, T, Cin, N, taps, pad_before=0, tokens=None, row_len=None, pool2=False, scale=None, shift=None,
                  rowbias=None, act=ACT_NONE, res=None, ldw=None, bf16=False, conv2d=None):
    """Returns (y [B*T, N], m [B*T, N]) in float64.  w is [taps*Cin, ldw] (ldw >= N, columns past N ignored); res [B*T, N];
    conv2d = dict(H, W, kh, kw, stride, pad_h, pad_w, Wo[, xb]) for the 2-D mode (T = Ho*Wo, taps = kh*kw)."""
    ldw = N if ldw is None else ldw
    w = np.asarray(w, dtype=np.float64).reshape(taps * Cin, ldw)[:, :N]
    if bf16:
        w = bf16_round(w.astype(np.float32)).astype(np.float64)
    if conv2d is not None:
        c = conv2d
        Ho = T // c["Wo"]
        assert Ho * c["Wo"] == T and c["kh"] * c["kw"] == taps
        cols = gather_rows_2d(x, B, c["H"], c["W"], Cin, c["kh"], c["kw"], c["stride"], c["pad_h"], c["pad_w"], Ho, c["Wo"],
                              c.get("xb"))
    else:
        cols = gather_rows(x, B, T, Cin, taps, pad_before, tokens, row_len, pool2)
    acc = np.zeros((B * T, N))
    mag = np.zeros((B * T, N))
    aw = np.abs(w)
    for j, g in enumerate(cols):
        g = g.reshape(B * T, Cin)
        if bf16:
            g = bf16_round(g.astype(np.float32)).astype(np.float64)
        wj = w[j * Cin:(j + 1) * Cin]
        acc += g @ wj
        mag += np.abs(g) @ aw[j * Cin:(j + 1) * Cin]
    sc = np.ones(N) if scale is None else np.asarray(scale, dtype=np.float64)
    sh = np.zeros(N) if shift is None else np.asarray(shift, dtype=np.float64)
    y = acc * sc + sh
    m = mag * np.abs(sc) + np.abs(sh)
    if rowbias is not None:
        rb = np.repeat(np.asarray(rowbias, dtype=np.float64).reshape(B, N), T, axis=0)
        y = y + rb
        m = m + np.abs(rb)
    if act == ACT_RELU:
        y = np.maximum(y, 0.0)
    elif act == ACT_TANH:
        y = np.tanh(y)
    if res is not None:
        y = y + np.asarray(res, dtype=np.float64).reshape(B * T, N)
    return y, m


def conv_gemm_naive(x, w, B, T, Cin, N, taps, pad_before=0, tokens=None, row_len=None, pool2=False, scale=None, shift=None,
                    rowbias=None, act=ACT_NONE, res=None):
    """The 1-D contract as plain loops (tiny shapes only): the check of conv_gemm_ref."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(taps * Cin, -1)
    table = x.reshape(-1, Cin)
    y = np.zeros((B * T, N))

    def row(b, s):
        r = tokens[b][s] if tokens is not None else b * T + s
        return table[r]

    for b in range(B):
        ln = T if row_len is None else min(T, int(row_len[b]))
        for t in range(T):
            for n in range(N):
                acc = 0.0
                for j in range(taps):
                    s = t + j - pad_before
                    if not 0 <= s < ln:
                        continue
                    for c in range(Cin):
                        v = row(b, s)[c]
                        if pool2 and s + 1 < ln:
                            v = max(v, row(b, s + 1)[c])
                        acc += v * w[j * Cin + c, n]
                v = acc * (1.0 if scale is None else scale[n]) + (0.0 if shift is None else shift[n])
                if rowbias is not None:
                    v += rowbias[b][n]
                if act == ACT_RELU:
                    v = max(v, 0.0)
                elif act == ACT_TANH:
                    v = np.tanh(v)
                if res is not None:
                    v += res[b * T + t][n]
                y[b * T + t, n] = v
    return y
