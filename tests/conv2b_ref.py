"""Literal numpy statements of the contracts of dtfill_conv2d_strided_backward_data / _weights and
dtfill_conv2d_transpose_backward_data / _weights (include/dtfill.h), for the tests only.  They extend convb_ref (g, the flipped
kernel, the segments and level 2's order) and conv2_ref (the forward chains the input gradients are) by importing them; what is
new here is the exchanged kernel, the spread of the 1x1 stride-2 layer, and level 1 over an output frame at a stride and over
the transposed layer's input frame.  The product does not import this file.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import conv2_ref as R2
import conv_ref as R
import convb_ref as RB

F = np.float32
ROWS, COLS = RB.CONV_BW_ROWS, RB.CONV_BW_COLS
g_ref = RB.g_ref  # dresidual is g itself


def exchanged(w):
    """wX[ky, kx, o, c] = w[ky, kx, c, o]: the channel axes exchanged, no flip."""
    return np.ascontiguousarray(np.asarray(w, F).transpose(0, 1, 3, 2))


def strided_dx_ref(dy, y, w, stride, act, alpha=0.2):
    """dy, y [B,Ho,Wo,Cout], w [ksize,ksize,Cin,Cout] -> dx [B,stride Ho,stride Wo,Cin] (stride 2: the even frame)."""
    g = g_ref(dy, y, act, alpha)
    ksize = w.shape[0]
    if stride == 1:
        return R2.strided_ref(g, RB.flipped(w))
    if ksize == 3:
        return R2.transpose_ref(g, exchanged(w))
    assert ksize == 1
    B, Ho, Wo, _ = g.shape
    dx = np.zeros((B, 2 * Ho, 2 * Wo, w.shape[2]), F)  # +0 off the even grid, whatever g holds
    dx[:, ::2, ::2] = R2.strided_ref(g, exchanged(w))  # the single tap (0, 0): a chain over o
    return dx


def transpose_dx_ref(dy, y, w_packed, act, alpha=0.2):
    """dy, y [B,2H,2W,Cout], w_packed [3,3,Cin,Cout] -> dx [B,H,W,Cin]."""
    return R2.strided_ref(g_ref(dy, y, act, alpha), exchanged(w_packed), stride=2)


def windows(a, ksize, stride, Ho, Wo, pt, pl):
    """win[b, h, v] = a[b, stride h + i - pt, stride v + j - pl, :] as [ksize, ksize, C], +0 outside the frame."""
    a = np.asarray(a, F)
    _, H, W, _ = a.shape
    pb = max(stride * (Ho - 1) + ksize - pt - H, 0)
    pr = max(stride * (Wo - 1) + ksize - pl - W, 0)
    ap = np.pad(a, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    win = sliding_window_view(ap, (ksize, ksize), axis=(1, 2))[:, ::stride, ::stride][:, :Ho, :Wo]
    return win.transpose(0, 1, 2, 4, 5, 3)


def _level1(frame, rows, cols, order, step, acc):
    """acc[segment] = step(acc[segment], b, h, v) for the pixels of every segment of `frame` = (B, H, W) in raster order: the
    segments are independent, so link k of all of them is one call."""
    B, H, W = frame
    segs = RB.segments(B, H, W, rows, cols, order)
    sb, h0, h1, v0, v1 = (np.array(c) for c in zip(*segs))
    for dh in range(min(rows, H)):
        for dv in range(min(cols, W)):
            on = np.nonzero((h0 + dh < h1) & (v0 + dv < v1))[0]
            if on.size:
                acc[on] = step(acc[on], sb[on], h0[on] + dh, v0[on] + dv)
    return acc


def _level2(part):
    total = np.zeros(part.shape[1:], F)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in part:
            total = total + p
    return total


def strided_partials(x, g, ksize, stride, rows=ROWS, cols=COLS, order="bts"):
    """Level 1 over the OUTPUT frame: float32 [segments, ksize^2 Cin + 1, Cout], the last row db's (a = 1.0)."""
    x, g = np.asarray(x, F), np.asarray(g, F)
    B, H, W, cin = x.shape
    (Ho, pt, _), (Wo, pl, _) = R2.same_rule(H, ksize, stride), R2.same_rule(W, ksize, stride)
    assert g.shape[:3] == (B, Ho, Wo)
    win = windows(x, ksize, stride, Ho, Wo, pt, pl)

    def step(acc, b, h, v):
        a = np.concatenate([win[b, h, v].reshape(b.size, -1), np.ones((b.size, 1), F)], axis=1)
        return R.fma32(a[:, :, None], g[b, h, v][:, None, :], acc)

    nseg = len(RB.segments(B, Ho, Wo, rows, cols))
    return _level1((B, Ho, Wo), rows, cols, order, step, np.zeros((nseg, ksize * ksize * cin + 1, g.shape[3]), F))


def strided_dw_ref(x, dy, y, ksize, stride, act, alpha=0.2, rows=ROWS, cols=COLS, order="bts"):
    """-> (dw [ksize,ksize,Cin,Cout], db [Cout]) of dtfill_conv2d_strided_backward_weights."""
    x = np.asarray(x, F)
    total = _level2(strided_partials(x, g_ref(dy, y, act, alpha), ksize, stride, rows, cols, order))
    return total[:-1].reshape(ksize, ksize, x.shape[3], -1).copy(), total[-1].copy()


def transpose_partials(x, g, rows=ROWS, cols=COLS, order="bts", db_chains=4):
    """Level 1 over the INPUT frame [H,W]: (dw partials [segments,3,3,Cin,Cout], db partials [segments,Cout]).  db_chains = 1 is
    the single raster chain over the segment's output pixels the four-chain order is told apart from in the tests."""
    x, g = np.asarray(x, F), np.asarray(g, F)
    B, H, W, cin = x.shape
    cout = g.shape[3]
    assert g.shape[:3] == (B, 2 * H, 2 * W)
    win = windows(g, 3, 2, H, W, 0, 0)  # [B,H,W,3,3,Cout]: g[b, 2 h + ky, 2 v + kx], +0 at row 2H and column 2W

    def step(acc, b, h, v):
        return R.fma32(x[b, h, v][:, None, None, :, None], win[b, h, v][:, :, :, None, :], acc)

    def step_q(q, b, h, v):
        return R.fma32(F(1), win[b, h, v][:, :2, :2], q)

    nseg = len(RB.segments(B, H, W, rows, cols))
    part = _level1((B, H, W), rows, cols, order, step, np.zeros((nseg, 3, 3, cin, cout), F))
    with np.errstate(over="ignore", invalid="ignore"):
        if db_chains == 4:
            q = _level1((B, H, W), rows, cols, order, step_q, np.zeros((nseg, 2, 2, cout), F))
            pb = ((q[:, 0, 0] + q[:, 0, 1]) + q[:, 1, 0]) + q[:, 1, 1]
        else:
            ones = np.ones((B, 2 * H, 2 * W, 1), F)
            full = strided_partials(ones, g, 1, 1, 2 * rows, 2 * cols, order)  # the same pixels as one raster chain
            pb = full[:, 1]
    return part, pb.astype(F)


def transpose_dw_ref(x, dy, y, act, alpha=0.2, rows=ROWS, cols=COLS, order="bts", db_chains=4):
    """-> (dw in the packed layout [3,3,Cin,Cout], db [Cout]) of dtfill_conv2d_transpose_backward_weights."""
    part, pb = transpose_partials(x, g_ref(dy, y, act, alpha), rows, cols, order, db_chains)
    return _level2(part), _level2(pb)
