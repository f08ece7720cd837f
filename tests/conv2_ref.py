"""Literal numpy statements of dtfill_conv2d_strided's and dtfill_conv2d_transpose's contracts (include/dtfill.h), for the tests
only, built on conv_ref's correctly rounded fma32 and its finish; and the float64 forms they are held to: a torch convolution of
an explicitly padded input, the vector-Jacobian product that defines the transposed convolution, and torch's conv_transpose2d.
The product does not import this file.
"""
import numpy as np

import conv_ref as C

F = np.float32
LINEAR, LEAKY = C.LINEAR, C.LEAKY


def same_rule(n, ksize, stride):
    """TensorFlow's 'same' rule for one axis: (output extent, padding in front, padding behind), the smaller half in front."""
    out = -(-n // stride)
    pad = max((out - 1) * stride + ksize - n, 0)
    return out, pad // 2, pad - pad // 2


def _finish(acc, bias, residual, act, alpha, residual_first=False):
    """acc + bias, + residual, activation: one rounded operation each.  residual_first is the order the contract is told apart
    from in the tests."""
    if residual is None:
        return C.finish(acc, bias, act, alpha)
    if residual_first:
        y = np.asarray(acc, F) + np.asarray(residual, F)
        return C.finish(y, bias, act, alpha)
    y = C.finish(acc, bias, LINEAR, alpha)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (y + np.asarray(residual, F)).astype(F)
    return C.finish(y, None, act, alpha)


def strided_ref(x, w, bias=None, stride=1, residual=None, act=LINEAR, alpha=0.2, residual_first=False):
    """x float32 [B,H,W,Cin], w [ksize,ksize,Cin,Cout] -> float32 [B,Ho,Wo,Cout]: dtfill_conv2d_strided's contract."""
    x, w = np.asarray(x, F), np.asarray(w, F)
    B, H, W, cin = x.shape
    ksize, _, _, cout = w.shape
    assert w.shape == (ksize, ksize, cin, cout) and stride in (1, 2)
    (Ho, pt, pb), (Wo, pl, pr) = same_rule(H, ksize, stride), same_rule(W, ksize, stride)
    xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    acc = np.zeros((B, Ho, Wo, cout), F)
    for i, j, c in C.chain_order(ksize, cin):
        acc = C.fma32(xp[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride, c:c + 1], w[i, j, c], acc)
    return _finish(acc, bias, residual, act, alpha, residual_first)


def parity_taps(parity):
    """The taps k of one axis with (y - k) even, y of the given parity, in order, each with how far back it reads: y = 2 a + 1
    reads x[a] under tap 1; y = 2 a reads x[a] under tap 0, then x[a - 1] under tap 2."""
    return [(1, 0)] if parity else [(0, 0), (2, 1)]


def transpose_ref(x, w, bias=None, act=LINEAR, alpha=0.2):
    """x float32 [B,H,W,Cin], w [3,3,Cin,Cout] (the ABI's layout) -> float32 [B,2H,2W,Cout]: dtfill_conv2d_transpose's contract."""
    x, w = np.asarray(x, F), np.asarray(w, F)
    B, H, W, cin = x.shape
    cout = w.shape[3]
    assert w.shape == (3, 3, cin, cout)
    xp = np.pad(x, ((0, 0), (1, 0), (1, 0), (0, 0)))  # index -1: one row above, one column to the left
    out = np.zeros((B, 2 * H, 2 * W, cout), F)
    for py in (0, 1):
        for px in (0, 1):
            acc = np.zeros((B, H, W, cout), F)
            for g in range(0, cin, C.GROUP):
                for ky, by in parity_taps(py):
                    for kx, bx in parity_taps(px):
                        for c in range(g, min(g + C.GROUP, cin)):
                            acc = C.fma32(xp[:, 1 - by:1 - by + H, 1 - bx:1 - bx + W, c:c + 1], w[ky, kx, c], acc)
            out[:, py::2, px::2] = C.finish(acc, bias, act, alpha)
    return out


def pack(kernel):
    """Keras's Conv2DTranspose.kernel [3,3,Cout,Cin] -> the ABI's [3,3,Cin,Cout]."""
    return np.ascontiguousarray(np.asarray(kernel).transpose(0, 1, 3, 2))


# ---- float64 forms ------------------------------------------------------------------------------------------------

def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _leaky64(y, act, alpha):
    return np.where(y > 0, y, y * np.float64(F(alpha))) if act == LEAKY else y


def strided_f64(x, w, bias=None, stride=1, residual=None, act=LINEAR, alpha=0.2):
    """float64 torch conv2d, padding 0, of the input padded as the 'same' rule says."""
    import torch

    ksize = w.shape[0]
    (_, pt, pb), (_, pl, pr) = same_rule(x.shape[1], ksize, stride), same_rule(x.shape[2], ksize, stride)
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    y = torch.nn.functional.conv2d(_t(xp).permute(0, 3, 1, 2), _t(w).permute(3, 2, 0, 1), None if bias is None else _t(bias),
                                   stride=stride).permute(0, 2, 3, 1).numpy()
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return _leaky64(y, act, alpha)


def transpose_f64_vjp(x, kernel, bias=None, act=LINEAR, alpha=0.2):
    """The definition: the gradient, with respect to its [B,2H,2W,Cout] input, of the stride-2 3x3 convolution under the Keras
    kernel [3,3,Cout,Cin] -- 'same' there pads one row below and one column to the right -- with x as the cotangent."""
    import torch

    B, H, W, cin = x.shape
    cout = kernel.shape[2]
    z = torch.zeros((B, cout, 2 * H, 2 * W), dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(z, (0, 1, 0, 1)), _t(kernel).permute(3, 2, 0, 1), stride=2)
    assert tuple(y.shape) == (B, cin, H, W)
    (grad,) = torch.autograd.grad(y, z, _t(x).permute(0, 3, 1, 2))
    out = grad.permute(0, 2, 3, 1).numpy()
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
    return _leaky64(out, act, alpha)


def transpose_f64_torch(x, kernel, bias=None, act=LINEAR, alpha=0.2):
    """torch.nn.functional.conv_transpose2d(stride=2), [B,2H+1,2W+1,Cout], cropped to [:2H, :2W]."""
    import torch

    B, H, W, _ = x.shape
    y = torch.nn.functional.conv_transpose2d(_t(x).permute(0, 3, 1, 2), _t(kernel).permute(3, 2, 0, 1),
                                             None if bias is None else _t(bias), stride=2)
    return _leaky64(y.permute(0, 2, 3, 1).numpy()[:, :2 * H, :2 * W], act, alpha)


def abs_sum_strided(x, w, bias=None, stride=1, residual=None):
    """sum |x| |w| + |bias| + |residual| per output, in float64."""
    total = strided_f64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), stride=stride)
    total = total + (0 if bias is None else np.abs(np.asarray(bias, np.float64)))
    return total + (0 if residual is None else np.abs(np.asarray(residual, np.float64)))


def abs_sum_transpose(x, kernel, bias=None):
    total = transpose_f64_torch(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(kernel, np.float64)))
    return total + (0 if bias is None else np.abs(np.asarray(bias, np.float64)))
