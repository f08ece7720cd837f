"""Numpy statements of the contracts of dtfill_conv2d_strided_backward_data_bf16 / _weights_bf16 and
dtfill_conv2d_transpose_backward_data_bf16 / _weights_bf16 (include/dtfill.h), for the tests only: bf16 rounding from
conv_bf16_ref, g from conv2b_ref (float32: a compare and one rounded product), the exact sums of the rounded operands in float64
or int64, beside them S = sum |x^| |g^| and the terms of the bounds.  The product does not import this file.
"""
import numpy as np

import conv2_ref as R2
import conv2b_ref as RW
import conv_bf16_ref as RH
import convb_ref as RB

F = np.float32
ROWS, COLS = RB.CONV_BW_ROWS, RB.CONV_BW_COLS
KSTEP = 32  # pixels of a k-step of the weight sum: the k of v_mfma_f32_16x16x32_bf16
TINY = RH.TINY
g_ref = RW.g_ref  # dresidual is g itself, exactly


def dx_kernel(w, stride, transposed):
    """The float32 kernel the data gradient's forward over g runs under: flipped at stride 1, exchanged otherwise."""
    return RW.exchanged(w) if transposed or stride == 2 else RB.flipped(w)


def dx_sum(g, w, stride, transposed=False, dtype=np.float64):
    """sum g w over the data gradient's terms, in `dtype`, of operands taken as they are: [B,H,W,Cin].  g [B,Ho,Wo,Cout]
    ([B,2H,2W,Cout] of the transposed layer), w the layer's [ksize,ksize,Cin,Cout]."""
    g, k = np.asarray(g, dtype), np.asarray(dx_kernel(np.asarray(w), stride, transposed), dtype)
    if transposed:
        return RH.strided_sum(g, k, 2, dtype)
    if stride == 1:
        return RH.strided_sum(g, k, 1, dtype)
    if w.shape[0] == 3:
        return RH.transpose_sum(g, k, dtype)
    B, Ho, Wo, _ = g.shape
    dx = np.zeros((B, 2 * Ho, 2 * Wo, w.shape[2]), dtype)  # +0 off the even grid
    dx[:, ::2, ::2] = RH.strided_sum(g, k, 1, dtype)
    return dx


def dx_ref(dy, y, w, stride, act, alpha=0.2, transposed=False):
    """-> (dx float64, the exact sum of g^ w^; S float64; n of the bound)."""
    gr, wr = RH.bf16_round(g_ref(dy, y, act, alpha)), RH.bf16_round(w)
    with np.errstate(over="ignore", invalid="ignore"):
        return (dx_sum(gr, wr, stride, transposed), dx_sum(np.abs(gr), np.abs(wr), stride, transposed),
                RH.bound_terms(w.shape[0], w.shape[3]))


def dx_bound(S, n):
    """dtfill_conv2d_strided_bf16's bound (b) without a bias or a residual."""
    return 2.0 * n * 2.0 ** -23 * S + n * TINY


def dw_sum(x, g, ksize, stride, transposed=False, dtype=np.float64):
    """(dw [ksize,ksize,Cin,Cout], db [Cout]): the sums of x g and of g over all pixels in `dtype`, operands as they are.
    x [B,H,W,Cin]; g over the output frame."""
    x, g = np.asarray(x, dtype), np.asarray(g, dtype)
    B, H, W, cin = x.shape
    cout = g.shape[3]
    if transposed:
        win = RW.windows(g.astype(np.float64), 3, 2, H, W, 0, 0).astype(dtype)  # [B,H,W,3,3,Cout], +0 at row 2H and column 2W
        dw = np.tensordot(x.reshape(-1, cin).T, win.reshape(B * H * W, 9 * cout), axes=1)  # [Cin, 9 Cout]
        dw = dw.reshape(cin, 3, 3, cout).transpose(1, 2, 0, 3)
    else:
        (Ho, pt, _), (Wo, pl, _) = R2.same_rule(H, ksize, stride), R2.same_rule(W, ksize, stride)
        assert g.shape[:3] == (B, Ho, Wo)
        win = RW.windows(x.astype(np.float64), ksize, stride, Ho, Wo, pt, pl).astype(dtype)  # [B,Ho,Wo,k,k,Cin]
        dw = np.tensordot(win.reshape(B * Ho * Wo, -1).T, g.reshape(-1, cout), axes=1).reshape(ksize, ksize, cin, cout)
    return np.ascontiguousarray(dw), g.reshape(-1, cout).sum(axis=0)


def bound_terms(frame, transposed_db=False):
    """n of the weight sum's bound over the small frame (B, H, W): the padded pixel count, every row of a segment as whole
    k-steps of 32, plus the number of segments.  The transposed layer's db has four chains a segment: four times as many."""
    B, H, W = frame
    segs_y, segs_x = -(-H // ROWS), -(-W // COLS)
    padded = 0
    for sx in range(segs_x):
        cols = min(COLS, W - sx * COLS)
        padded += H * KSTEP * -(-cols // KSTEP)
    n = B * padded + B * segs_y * segs_x
    return 4 * n if transposed_db else n


def small_frame(x_shape, stride, transposed):
    B, H, W = x_shape[:3]
    return (B, H, W) if transposed else (B, H // stride, W // stride)


def dw_ref(x, dy, y, ksize, stride, act, alpha=0.2, transposed=False):
    """-> (dw, db: the exact sums of x^ g^ and g^ in float64; bound_dw, bound_db: the contract's (b) per element)."""
    xr, gr = RH.bf16_round(x), RH.bf16_round(g_ref(dy, y, act, alpha))
    with np.errstate(over="ignore", invalid="ignore"):
        dw, db = dw_sum(xr, gr, ksize, stride, transposed)
        Sw, Sb = dw_sum(np.abs(xr), np.abs(gr), ksize, stride, transposed)
    frame = small_frame(x.shape, stride, transposed)
    n, nb = bound_terms(frame), bound_terms(frame, transposed)
    return dw, db, 2.0 * n * 2.0 ** -23 * Sw + n * TINY, 2.0 * nb * 2.0 ** -23 * Sb + nb * TINY


def integer_case(ksize, stride, cin, cout, frame, seed, transposed=False):
    """x in [-8, 8], dy in [-3, 3], w in [-4, 4], all integers, y of either sign with a few -0; under leaky with alpha = 0.25
    every operand is exact in bf16 and every partial sum is a multiple of 2^-4 far below 2^24: exact in any order.
    frame: the small frame (B, Hs, Ws).  Returns x, w, dy, y (float32)."""
    rng = np.random.default_rng(seed)
    B, Hs, Ws = frame
    xs = (B, Hs, Ws) if transposed else (B, stride * Hs, stride * Ws)
    ys = (B, 2 * Hs, 2 * Ws) if transposed else (B, Hs, Ws)
    x = rng.integers(-8, 9, xs + (cin,)).astype(F)
    w = rng.integers(-4, 5, (ksize, ksize, cin, cout)).astype(F)
    dy = rng.integers(-3, 4, ys + (cout,)).astype(F)
    y = rng.standard_normal(ys + (cout,)).astype(F)
    y[rng.random(y.shape) < 0.05] = -0.0
    return x, w, dy, y


ALPHA_INT = 0.25


def integer_ref(x, w, dy, y, stride, act, transposed=False):
    """(dx, dresidual, dw, db) of an integer_case in int64 arithmetic on 4 g, as float32: the exact values."""
    g = g_ref(dy, y, act, ALPHA_INT)
    g4 = np.rint(g.astype(np.float64) * 4).astype(np.int64)
    assert np.array_equal(g4 / 4.0, g.astype(np.float64))
    for a in (x, w, g):
        assert np.array_equal(RH.bf16_round(a), np.asarray(a, F)), "an operand is not exact in bf16"
    xi, wi = np.rint(x).astype(np.int64), np.rint(w).astype(np.int64)
    dx = dx_sum(g4, wi, stride, transposed, np.int64)
    dw, db = dw_sum(xi, g4, w.shape[0], stride, transposed, np.int64)
    for a in (dx, dw, db):
        assert np.abs(a).max() < 2 ** 24
    return (dx / 4.0).astype(F), g, (dw / 4.0).astype(F), (db / 4.0).astype(F)
