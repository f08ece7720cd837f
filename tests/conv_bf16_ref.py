"""Numpy statements of dtfill_conv2d_strided_bf16's, dtfill_conv2d_transpose_bf16's and dtfill_conv2d_pack_bf16's contracts
(include/dtfill.h), for the tests only: the operands rounded to bf16, the sum of the exact products in float64 (and in int64
for the exact cases), beside it S = sum |bf16(x)| |bf16(w)|, and the float32 finish as conv2_ref has it.  The product does not
import this file.
"""
import numpy as np

import conv2_ref as R2

F = np.float32
GROUP = 32  # input channels per group: one k-step of the bf16 MFMA


def bf16_round(a):
    """float32 -> the nearest bf16, ties to even, as float32: on the bit pattern.  NaN stays NaN (quieted, sign kept); a value
    past the largest finite bf16 goes to +-inf."""
    a = np.ascontiguousarray(a, dtype=F)
    bits = a.view(np.uint32).astype(np.uint64)
    rounded = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    out = np.where(nan, (bits | 0x00400000) & 0xFFFF0000, rounded).astype(np.uint32)
    return out.view(F).reshape(a.shape)


def bf16_bits(a):
    """The 16 bits of bf16_round(a)."""
    return (bf16_round(a).view(np.uint32) >> 16).astype(np.uint16)


def bound_terms(ksize, cin):
    """n of the contract's bound: the addends of one output's MFMAs, padded half groups included."""
    return ksize * ksize * GROUP * -(-cin // GROUP)


def strided_sum(x, w, stride, dtype=np.float64):
    """sum x w over the taps and channels of dtfill_conv2d_strided's contract, in `dtype`: [B,Ho,Wo,Cout]."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    B, H, W, cin = x.shape
    ksize, cout = w.shape[0], w.shape[3]
    assert w.shape == (ksize, ksize, cin, cout) and stride in (1, 2)
    (Ho, pt, pb), (Wo, pl, pr) = R2.same_rule(H, ksize, stride), R2.same_rule(W, ksize, stride)
    xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    acc = np.zeros((B, Ho, Wo, cout), dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(ksize):
            for j in range(ksize):
                acc += xp[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride] @ w[i, j]
    return acc


def transpose_sum(x, w, dtype=np.float64):
    """sum x w over the taps and channels of dtfill_conv2d_transpose's contract (w: the ABI's [3,3,Cin,Cout]): [B,2H,2W,Cout]."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    B, H, W, cin = x.shape
    cout = w.shape[3]
    assert w.shape == (3, 3, cin, cout)
    xp = np.pad(x, ((0, 0), (1, 0), (1, 0), (0, 0)))  # index -1: one row above, one column to the left
    out = np.zeros((B, 2 * H, 2 * W, cout), dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for py in (0, 1):
            for px in (0, 1):
                for ky, by in R2.parity_taps(py):
                    for kx, bx in R2.parity_taps(px):
                        out[:, py::2, px::2] += xp[:, 1 - by:1 - by + H, 1 - bx:1 - bx + W] @ w[ky, kx]
    return out


def _finished(total, bias, residual, act, alpha):
    with np.errstate(over="ignore", invalid="ignore"):
        return R2._finish(total.astype(F), bias, residual, act, alpha)


def conv2d_strided_bf16_ref(x, w, bias=None, stride=1, residual=None, act=R2.LINEAR, alpha=0.2):
    """-> (out float32 [B,Ho,Wo,Cout], S float64): the float64 sum of bf16(x) bf16(w), finished in float32; S = sum |..| |..|."""
    xr, wr = bf16_round(x), bf16_round(w)
    return _finished(strided_sum(xr, wr, stride), bias, residual, act, alpha), strided_sum(np.abs(xr), np.abs(wr), stride)


def conv2d_transpose_bf16_ref(x, w, bias=None, act=R2.LINEAR, alpha=0.2):
    """-> (out float32 [B,2H,2W,Cout], S float64); w: the ABI's [3,3,Cin,Cout]."""
    xr, wr = bf16_round(x), bf16_round(w)
    return _finished(transpose_sum(xr, wr), bias, None, act, alpha), transpose_sum(np.abs(xr), np.abs(wr))


def bound(ksize, cin, S, bias=None, residual=None):
    """The contract's bound (b) per output: 2 n 2^-23 (S + |bias| + |residual|) + n 2^-149."""
    total = S + (0 if bias is None else np.abs(np.asarray(bias, np.float64)))
    total = total + (0 if residual is None else np.abs(np.asarray(residual, np.float64)))
    return 2.0 * bound_terms(ksize, cin) * 2.0 ** -23 * total + bound_terms(ksize, cin) * TINY


TINY = 2.0 ** -149  # the absolute term's unit: a product below 2^-126 is rounded once, to a multiple of 2^-149


def packed_elems(ksize, cin, cout):
    return ksize * ksize * -(-cin // GROUP) * (cout // 16) * 512


def pack_ref(w):
    """w float32 [ksize,ksize,Cin,Cout] -> uint16 [ksize^2 G N 512], the header's layout: element
    (((T G + g) N + n) 64 + 16 kq + m) 8 + j holds bf16(w[T][32 g + 8 kq + j][16 n + m]), +0 past Cin."""
    w = np.asarray(w, F)
    ksize, _, cin, cout = w.shape
    G, N = -(-cin // GROUP), cout // 16
    padded = np.zeros((ksize * ksize, G * GROUP, cout), np.uint16)
    padded[:, :cin] = bf16_bits(w).reshape(ksize * ksize, cin, cout)
    # [T][g][kq][j][n][m] -> [T][g][n][kq][m][j]
    return np.ascontiguousarray(padded.reshape(ksize * ksize, G, 4, 8, N, 16).transpose(0, 1, 4, 2, 5, 3)).reshape(-1)
