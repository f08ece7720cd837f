"""A literal numpy statement of the contracts of dtfill_conv2d_backward_data and dtfill_conv2d_backward_weights
(include/dtfill.h), for the tests only, built from conv_ref's fma32: the activation's derivative g, dx as dtfill_conv2d's own
chain over g under the flipped kernel, and dw / db as a two-level sum: a partial fmaf chain per segment over its pixels in
raster order, then the partials added in (b, t, s) order from +0.  The product does not import this file.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import conv_ref as R

F = np.float32
CONV_BW_ROWS, CONV_BW_COLS = 32, 64  # DTFILL_CONV_BW_ROWS, DTFILL_CONV_BW_COLS of include/dtfill.h: a segment


def g_ref(dy, y, act, alpha=0.2):
    """g = y > 0 ? dy : dy * alpha (one rounded multiply), dy itself for a linear layer.  y == +-0 and NaN take the alpha branch."""
    dy = np.asarray(dy, F)
    if act != R.LEAKY:
        return dy.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(np.asarray(y, F) > 0, dy, dy * F(alpha)).astype(F)


def flipped(w):
    """wT[i, j, o, c] = w[ksize - 1 - i, ksize - 1 - j, c, o]."""
    return np.ascontiguousarray(np.asarray(w, F)[::-1, ::-1].transpose(0, 1, 3, 2))


def dx_ref(dy, y, w, act, alpha=0.2):
    """dy, y [B,H,W,Cout], w [ksize,ksize,Cin,Cout] -> dx [B,H,W,Cin]: conv_ref's chain over g under wT, no bias, no activation."""
    return R.conv_ref(g_ref(dy, y, act, alpha), flipped(w))


def segments(B, H, W, rows=CONV_BW_ROWS, cols=CONV_BW_COLS, order="bts"):
    """The segments (b, h0, h1, v0, v1) of a batch, cut at the frame's edges, in level 2's order: "bts" is the contract, frame
    outermost, then the segment rows, then the segment columns; "stb" is the reverse nesting the tests tell it apart from."""
    nt, ns = -(-H // rows), -(-W // cols)
    if order == "bts":
        keys = [(b, t, s) for b in range(B) for t in range(nt) for s in range(ns)]
    else:
        keys = [(b, t, s) for s in range(ns) for t in range(nt) for b in range(B)]
    return [(b, rows * t, min(rows * t + rows, H), cols * s, min(cols * s + cols, W)) for b, t, s in keys]


def partials(x, g, ksize, rows=CONV_BW_ROWS, cols=CONV_BW_COLS, order="bts"):
    """Level 1.  x [B,H,W,Cin], g [B,H,W,Cout] -> float32 [segments, ksize^2 Cin + 1, Cout] in segments()'s order: row
    (i ksize + j) Cin + c is dw[i, j, c, :]'s partial, the last row db's (a = 1.0).  Every segment's chain runs over its own
    pixels in raster order; the segments are independent, so step k of all of them is one fma32 call."""
    x, g = np.asarray(x, F), np.asarray(g, F)
    B, H, W, cin = x.shape
    cout = g.shape[3]
    r = (ksize - 1) // 2
    # win[b, h, v] = x[b, h - r .. h + r, v - r .. v + r, :] as [ksize, ksize, Cin], +0 outside the frame
    win = sliding_window_view(R.padded(x, r), (ksize, ksize), axis=(1, 2)).transpose(0, 1, 2, 4, 5, 3)
    segs = segments(B, H, W, rows, cols, order)
    sb, h0, h1, v0, v1 = (np.array(c) for c in zip(*segs))
    acc = np.zeros((len(segs), ksize * ksize * cin + 1, cout), F)
    for dh in range(min(rows, H)):
        for dv in range(min(cols, W)):
            on = np.nonzero((h0 + dh < h1) & (v0 + dv < v1))[0]
            if not on.size:
                continue
            b, h, v = sb[on], h0[on] + dh, v0[on] + dv
            a = np.concatenate([win[b, h, v].reshape(on.size, -1), np.ones((on.size, 1), F)], axis=1)
            acc[on] = R.fma32(a[:, :, None], g[b, h, v][:, None, :], acc[on])
    return acc


def dw_ref(x, dy, y, ksize, act, alpha=0.2, rows=CONV_BW_ROWS, cols=CONV_BW_COLS, order="bts"):
    """-> (dw float32 [ksize,ksize,Cin,Cout], db float32 [Cout]): level 2 over partials(), one rounded float32 add a segment."""
    x = np.asarray(x, F)
    part = partials(x, g_ref(dy, y, act, alpha), ksize, rows, cols, order)
    total = np.zeros(part.shape[1:], F)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in part:
            total = total + p
    return total[:-1].reshape(ksize, ksize, x.shape[3], -1).copy(), total[-1].copy()
