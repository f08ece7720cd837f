"""The convolutions on the device: one layer's forward and backward as functions of tensors, in the fixed float32 summation
orders of include/dtfill.h.  There are four KINDS of layer, and _KINDS states once what tells them apart (the ABI's symbols, the
frame arithmetic, the arguments only that kind takes):

  narrow      dtfill_conv2d            stride-1 'same', few output channels, x may be a [B,H,W] plane (SparsityCNN's layers)
  strided     dtfill_conv2d_strided    'same' at stride 1 or 2, many channels, an optional residual add (ResNet18's)
  transposed  dtfill_conv2d_transpose  Conv2DTranspose(Cout, 3, strides=2) on the packed kernel (pack_transpose_kernel)
  image       dtfill_conv2d_image      stride-1 'same' on an image of 2 to 4 channels; no data gradient, the image is data

Three cores hold the checks, the frames, the outputs, the workspace and the ABI call once, under a kind: _forward,
_backward_data and _backward_weights.  The public functions are one-line calls of them, each with its own signature and
docstring: conv2d_device, conv2d_strided_device, conv2d_transpose_device and conv2d_image_device forward; the seven
*_backward_data_device and *_backward_weights_device; the three *_workspace_bytes size functions.  autograd.py's convolution
calls the cores directly with the kind it carries.  conv2d_strided, conv2d_transpose and conv2d_image are the numpy forms
(tools.conv2d is the narrow one's).

The strided and the transposed kind have a second forward, on the bf16 matrix cores with float32 accumulation
(dtfill_conv2d_strided_bf16, dtfill_conv2d_transpose_bf16: the header states what is promised about its bits): pack_bf16_device
makes the packed weights once, conv2d_strided_bf16_device and conv2d_transpose_bf16_device take them in place of w through one
core, _forward_bf16, under the same _KINDS record; conv2d_strided_bf16 and conv2d_transpose_bf16 are the numpy forms.  Their
backward on the same matrix cores (dtfill_conv2d_strided_backward_data_bf16 and its three siblings) goes through
_backward_data and _backward_weights under precision = "bf16", which the _KINDS record maps to the symbols and the size
function: conv2d_strided_backward_data_bf16_device and the other three *_bf16_device functions, and their numpy forms without
the suffix _device.  They take the plain float32 w, not the packed one: the weights change every step and the call packs them.

The *_device functions and the size functions are reached as device.<name> as well, and everything here as net.<name>; they live
here, beside device.py's helpers, as the pools do in pool.py.  Their argument checks are held by tests/test_conv2d*.py, the
kernels by tests/test_gpu_conv2d*.py.
"""
import collections

import numpy as np
import torch

from . import _lib
from . import device as _device
from .device import _check_tensor, _ptr, _require_gpu, _stream


def _check_act(act, alpha=0.0):
    """The activation of a convolution, and with alpha that of its backward, which takes the derivative by the sign of the
    output; then the device, so that nothing below starts without one."""
    if act not in _lib.CONV_ACTS:
        raise ValueError("act must be one of %s, got %r" % (sorted(_lib.CONV_ACTS), act))
    if not alpha >= 0:
        raise ValueError("alpha must be >= 0 (the derivative is taken by the sign of the output), got %r" % (alpha,))
    _require_gpu()


def _check_conv_args(x, w, bias, act, what, plane_ok=False):
    """The checks the convolutions share; returns (B, H, W, Cin, Cout).  plane_ok: x may be [B,H,W], which is Cin = 1."""
    _check_act(act)
    if plane_ok and x.dim() == 3:
        _check_tensor(x, "x")
    else:
        _check_tensor(x, "x", layout="[B,H,W,Cin]")
    B, H, W = x.shape[:3]
    Cin = x.shape[3] if x.dim() == 4 else 1
    _check_tensor(w, "w", layout=what)
    if w.shape[0] != w.shape[1] or w.shape[2] != Cin or w.device != x.device:
        raise ValueError("w must be %s with Cin = %d on %s, got %s" % (what, Cin, x.device, tuple(w.shape)))
    Cout = w.shape[3]
    if bias is not None:
        _check_tensor(bias, "bias", layout="[Cout]")
        if bias.shape[0] != Cout or bias.device != x.device:
            raise ValueError("bias must be [%d] on %s, got %s" % (Cout, x.device, tuple(bias.shape)))
    return B, H, W, Cin, Cout


def _check_conv_out(x, out, out_offset, frame, Cout):
    """out of a convolution, [B,Ho,Wo,C] with frame = (B, Ho, Wo): a new [.., Cout] tensor when None."""
    if out is None:
        if out_offset != 0:
            raise ValueError("out_offset needs an out tensor to point into")
        return torch.empty(frame + (Cout,), dtype=torch.float32, device=x.device)
    _check_tensor(out, "out", layout="[B,Ho,Wo,C]")
    if tuple(out.shape[:3]) != frame or out.device != x.device:
        raise ValueError("out must be [%d,%d,%d,C] on %s, got %s" % (frame + (x.device, tuple(out.shape))))
    if out.data_ptr() == x.data_ptr():
        raise ValueError("out may not alias x")
    return out


_convb_ws = _device._Scratch()  # the workspace of the backward calls, of every kind of layer


def _check_conv_slice(t, what, like, offset, channels):
    """A gradient or an output of a layer as the backward reads it: [B,H,W,C] (or [B,H,W] as C = 1) with like's frames and
    device, of which the channels offset .. offset + channels - 1 are the layer's.  Returns C."""
    if t.dim() == 3:
        _check_tensor(t, what)
    else:
        _check_tensor(t, what, layout="[B,H,W,C]")
    C = t.shape[3] if t.dim() == 4 else 1
    if t.shape[:3] != like.shape[:3] or t.device != like.device:
        raise ValueError("%s must have the frames %s on %s, got %s" % (what, tuple(like.shape[:3]), like.device, tuple(t.shape)))
    if offset < 0 or offset + channels > C:
        raise ValueError("%s has %d channels: no room for %d at offset %d" % (what, C, channels, offset))
    return C


def _check_conv_backward(dy, y, act, dy_offset, y_offset, Cout):
    """dy and y as a layer's backward reads them; returns (dy's width, y or None for a linear layer, y's width)."""
    Cdy = _check_conv_slice(dy, "dy", dy, dy_offset, Cout)
    if act == "linear":
        return Cdy, None, 0
    if y is None:
        raise ValueError("the derivative of act = %r needs y, the forward's output" % act)
    return Cdy, y, _check_conv_slice(y, "y", dy, y_offset, Cout)


# What tells the four kinds of layer apart.  forward, data, weights: the ABI's symbols (data None: the image layer has no data
# gradient); abi_shape(ksize, Cout, stride): what they take between the tensors and act; has_residual: the forward takes a
# residual and the data call gives dresidual; ws_bytes(L, B, H, W, Cin, ksize, Cout, stride): the library's size function;
# ksize: the [3,3,..] rule, or None for any square kernel; plane_ok: x may be a [B,H,W] plane; out_frame(H, W, stride): the
# forward's output frame for ANY input frame (TensorFlow's 'same' rule, ceil(H / stride)); x_frame(Ho, Wo, stride): the
# forward's input frame under a dy of [Ho,Wo], and dy_frame(H, W, stride) the reverse, each None where the kind has no such
# layer (the backward's evenness rule).  ws_bytes_bf16: the size function of the backward under precision = "bf16", whose symbols
# are data and weights with "_bf16" appended; None where the kind has no such backward.
_Kind = collections.namedtuple("_Kind", "forward data weights abi_shape has_residual ws_bytes w_name w_layout ksize dy_layout "
                                        "plane_ok out_frame x_frame dy_frame ws_bytes_bf16", defaults=(None,))
PRECISIONS = ("float32", "bf16")
_KINDS = {
    "narrow": _Kind("dtfill_conv2d", "dtfill_conv2d_backward_data", "dtfill_conv2d_backward_weights",
                    lambda ksize, Cout, s: (ksize, Cout), False,
                    lambda L, B, H, W, Cin, ksize, Cout, s: L.dtfill_conv2d_backward_workspace_bytes(B, H, W, Cin, ksize, Cout),
                    "w", "[ksize,ksize,Cin,Cout]", None, "[B,H,W,C]", True,
                    lambda H, W, s: (H, W), lambda Ho, Wo, s: (Ho, Wo), lambda H, W, s: (H, W)),
    "strided": _Kind("dtfill_conv2d_strided", "dtfill_conv2d_strided_backward_data", "dtfill_conv2d_strided_backward_weights",
                     lambda ksize, Cout, s: (ksize, Cout, s), True,
                     lambda L, B, H, W, Cin, ksize, Cout, s: L.dtfill_conv2d_wide_backward_workspace_bytes(B, H, W, Cin, ksize, Cout, s, 0),
                     "w", "[ksize,ksize,Cin,Cout]", None, "[B,Ho,Wo,C]", False,
                     lambda H, W, s: (-(-H // s), -(-W // s)), lambda Ho, Wo, s: (s * Ho, s * Wo),
                     lambda H, W, s: None if H % s or W % s else (H // s, W // s),
                     lambda L, B, H, W, Cin, ksize, Cout, s: L.dtfill_conv2d_wide_backward_bf16_workspace_bytes(B, H, W, Cin, ksize, Cout, s, 0)),
    "transposed": _Kind("dtfill_conv2d_transpose", "dtfill_conv2d_transpose_backward_data", "dtfill_conv2d_transpose_backward_weights",
                        lambda ksize, Cout, s: (Cout,), False,
                        lambda L, B, H, W, Cin, ksize, Cout, s: L.dtfill_conv2d_wide_backward_workspace_bytes(B, H, W, Cin, 3, Cout, 2, 1),
                        "w_packed", "[3,3,Cin,Cout]", 3, "[B,2H,2W,C]", False,
                        lambda H, W, s: (2 * H, 2 * W), lambda Ho, Wo, s: None if Ho % 2 or Wo % 2 else (Ho // 2, Wo // 2),
                        lambda H, W, s: (2 * H, 2 * W),
                        lambda L, B, H, W, Cin, ksize, Cout, s: L.dtfill_conv2d_wide_backward_bf16_workspace_bytes(B, H, W, Cin, 3, Cout, 2, 1)),
    # the layer that reads the image: no data call, the image is data
    "image": _Kind("dtfill_conv2d_image", None, "dtfill_conv2d_image_backward_weights", lambda ksize, Cout, s: (ksize, Cout), False,
                   lambda L, B, H, W, Cin, ksize, Cout, s: L.dtfill_conv2d_image_backward_workspace_bytes(B, H, W, Cin, ksize, Cout),
                   "w", "[ksize,ksize,Cin,Cout]", None, "[B,H,W,C]", False,
                   lambda H, W, s: (H, W), lambda Ho, Wo, s: (Ho, Wo), lambda H, W, s: (H, W)),
}


def _check_frames(kind, x, Cout, stride, residual, out, out_offset):
    """The residual and out of a forward of `kind` against the output frame of x [B,H,W,..] at `stride`; returns out, a new
    [B,Ho,Wo,Cout] tensor when None."""
    k = _KINDS[kind]
    frame = (x.shape[0],) + k.out_frame(x.shape[1], x.shape[2], stride)
    if residual is not None:
        if not k.has_residual:
            raise ValueError("a %s layer takes no residual" % kind)
        _check_tensor(residual, "residual", layout="[B,Ho,Wo,Cout]")
        if tuple(residual.shape) != frame + (Cout,) or residual.device != x.device:
            raise ValueError("residual must be %s on %s, got %s" % (frame + (Cout,), x.device, tuple(residual.shape)))
    out = _check_conv_out(x, out, out_offset, frame, Cout)
    if residual is not None and out.data_ptr() == residual.data_ptr():
        raise ValueError("out may not alias residual")
    return out


def _forward(kind, x, w, bias, stride, residual, act, alpha, out, out_offset):
    """The forward of a layer of `kind`: the four public functions' shared sequence, once."""
    k = _KINDS[kind]
    if stride not in (1, 2):
        raise ValueError("stride must be 1 or 2, got %r" % (stride,))
    B, H, W, Cin, Cout = _check_conv_args(x, w, bias, act, k.w_layout, plane_ok=k.plane_ok)
    ksize = w.shape[0]
    if ksize != (k.ksize or ksize):
        raise ValueError("%s must be %s, got %s" % (k.w_name, k.w_layout, tuple(w.shape)))
    out = _check_frames(kind, x, Cout, stride, residual, out, out_offset)
    with torch.cuda.device(x.device):
        _lib.check(getattr(_lib.load(), k.forward)(
            x.data_ptr(), B, H, W, Cin, w.data_ptr(), _ptr(bias), *k.abi_shape(ksize, Cout, stride),
            *((_ptr(residual),) if k.has_residual else ()), _lib.CONV_ACTS[act], float(alpha), out.data_ptr(), out.shape[3],
            int(out_offset), _stream(x.device)))
    return out


def _check_backward_kind(kind, act, alpha, stride, precision="float32"):
    """Returns (the kind's record, the suffix of its backward symbols under `precision`, its size function)."""
    if precision not in PRECISIONS:
        raise ValueError("precision must be one of %s, got %r" % (PRECISIONS, precision))
    k = _KINDS[kind]
    if precision == "bf16" and k.ws_bytes_bf16 is None:
        raise ValueError("a %s layer has no bf16 backward" % kind)
    _check_act(act, alpha)
    if stride not in (1, 2):
        raise ValueError("stride must be 1 or 2, got %r" % (stride,))
    return (k, "_bf16", k.ws_bytes_bf16) if precision == "bf16" else (k, "", k.ws_bytes)


def _backward_data(kind, dy, w, stride, y, act, alpha, dy_offset, y_offset, dx, dx_offset, want_residual=False, precision="float32"):
    """The data gradient of a layer of `kind`: the public functions' shared sequence, once."""
    k, suffix, ws_bytes = _check_backward_kind(kind, act, alpha, stride, precision)
    _check_tensor(w, k.w_name, layout=k.w_layout)
    ksize, Cin, Cout = w.shape[0], w.shape[2], w.shape[3]
    Cdy, y, Cy = _check_conv_backward(dy, y, act, dy_offset, y_offset, Cout)
    frame = k.x_frame(dy.shape[1], dy.shape[2], stride) if dy.dim() == 4 or k.plane_ok else None
    if frame is None or w.shape[1] != ksize or ksize != (k.ksize or ksize) or w.device != dy.device:
        raise ValueError("dy must be %s and %s %s on %s, got %s and %s"
                         % (k.dy_layout, k.w_name, k.w_layout, dy.device, tuple(dy.shape), tuple(w.shape)))
    B, (H, W) = dy.shape[0], frame
    dx = _check_conv_out(dy, dx, dx_offset, (B, H, W), Cin)
    if y is not None and dx.data_ptr() == y.data_ptr():
        raise ValueError("dx may not alias y")
    dres = torch.empty(tuple(dy.shape[:3]) + (Cout,), dtype=torch.float32, device=dy.device) if want_residual else None
    L = _lib.load()
    nbytes = _device._sized(ws_bytes(L, B, H, W, Cin, ksize, Cout, stride))
    with torch.cuda.device(dy.device):
        with _convb_ws.hold(dy.device, nbytes) as ws:
            _lib.check(getattr(L, k.data + suffix)(
                dy.data_ptr(), Cdy, int(dy_offset), _ptr(y), Cy, int(y_offset), w.data_ptr(), B, H, W, Cin,
                *k.abi_shape(ksize, Cout, stride), _lib.CONV_ACTS[act], float(alpha), dx.data_ptr(), dx.shape[3], int(dx_offset),
                *((_ptr(dres),) if k.has_residual else ()), ws, nbytes, _stream(dy.device)))
    return (dx, dres) if want_residual else dx


def _backward_weights(kind, x, dy, ksize, stride, y, act, alpha, dy_offset, y_offset, cout, want_bias, precision="float32"):
    """The weight and bias gradients of a layer of `kind`: the shared sequence, once."""
    k, suffix, ws_bytes = _check_backward_kind(kind, act, alpha, stride, precision)
    plane = k.plane_ok and x.dim() == 3
    _check_tensor(x, "x", layout="[B,H,W]" if plane else "[B,H,W,Cin]")
    B, H, W, Cin = (*x.shape, 1) if plane else x.shape
    frame = k.dy_frame(H, W, stride)
    if frame is None:
        raise ValueError("the backward of a stride-2 layer needs an even frame, got %d x %d" % (H, W))
    if (dy.dim() != 4 and not k.plane_ok) or dy.shape[:3] != (B, *frame) or x.device != dy.device:
        raise ValueError("dy must have the frames %s on %s, got %s" % ((B, *frame), x.device, tuple(dy.shape)))
    Cout = int(cout) if cout is not None else (dy.shape[3] if dy.dim() == 4 else 1)
    Cdy, y, Cy = _check_conv_backward(dy, y, act, dy_offset, y_offset, Cout)
    ksize = int(ksize)
    L = _lib.load()
    nbytes = _device._sized(ws_bytes(L, B, H, W, Cin, ksize, Cout, stride))
    dw = torch.empty((ksize, ksize, Cin, Cout), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if want_bias else None
    with torch.cuda.device(x.device):
        with _convb_ws.hold(x.device, nbytes) as ws:
            _lib.check(getattr(L, k.weights + suffix)(
                x.data_ptr(), dy.data_ptr(), Cdy, int(dy_offset), _ptr(y), Cy, int(y_offset), B, H, W, Cin,
                *k.abi_shape(ksize, Cout, stride), _lib.CONV_ACTS[act], float(alpha), dw.data_ptr(), _ptr(db), ws, nbytes,
                _stream(x.device)))
    return dw, db


def conv2d_device(x, w, bias=None, act="linear", alpha=0.2, out=None, out_offset=0):
    """A stride-1 'same' float32 convolution in the fixed summation order of include/dtfill.h, dtfill_conv2d (a layer of
    net.py's SparsityCNN).  x: contiguous float32 CUDA tensor [B,H,W,Cin], or [B,H,W] for Cin = 1; w: [ksize,ksize,Cin,Cout], a
    Keras Conv2D.kernel as stored (cross-correlation); bias: [Cout] or None; act: "linear" or "leaky" (y > 0 ? y : y * alpha).
    out: a contiguous float32 tensor [B,H,W,C] on x's device of which the channels out_offset .. out_offset + Cout - 1 are
    written and the others left as they are (not x itself); a new [B,H,W,Cout] tensor by default.  Returns out.  Asynchronous on
    the current stream; the shapes the library takes are the header's (DtfillError otherwise)."""
    return _forward("narrow", x, w, bias, 1, None, act, alpha, out, out_offset)


def conv2d_backward_workspace_bytes(B, H, W, Cin, ksize, Cout):
    """The bytes of workspace either backward call of a layer needs (dtfill_conv2d_backward_workspace_bytes): host arithmetic,
    no device.  DtfillError for a shape outside dtfill_conv2d's domain."""
    return _device._sized(_lib.load().dtfill_conv2d_backward_workspace_bytes(int(B), int(H), int(W), int(Cin), int(ksize), int(Cout)))


def conv2d_backward_data_device(dy, w, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0, dx=None, dx_offset=0):
    """The gradient of conv2d_device with respect to x, in the fixed order of include/dtfill.h, dtfill_conv2d_backward_data.
    dy: contiguous float32 CUDA tensor [B,H,W,C] (or [B,H,W], C = 1), the gradient of the layer's output in the channels
    dy_offset .. dy_offset + Cout - 1; w: the layer's [ksize,ksize,Cin,Cout]; y: the forward's output, read at y_offset likewise,
    needed unless act is "linear".  dx: a contiguous float32 tensor [B,H,W,C'] of which the channels dx_offset .. dx_offset +
    Cin - 1 are written; a new [B,H,W,Cin] tensor by default.  Returns dx.  Asynchronous on the current stream."""
    return _backward_data("narrow", dy, w, 1, y, act, alpha, dy_offset, y_offset, dx, dx_offset)


def conv2d_backward_weights_device(x, dy, ksize, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0, cout=None, want_bias=True):
    """The gradients of conv2d_device with respect to w and bias, in the fixed two-level order of include/dtfill.h,
    dtfill_conv2d_backward_weights.  x: the forward's input, [B,H,W,Cin] or [B,H,W]; dy, y, act, alpha and the offsets as in
    conv2d_backward_data_device; cout: the layer's output channels (default: all of dy's).  Returns (dw [ksize,ksize,Cin,Cout],
    db [Cout] or None without want_bias): new tensors.  Asynchronous on the current stream."""
    return _backward_weights("narrow", x, dy, ksize, 1, y, act, alpha, dy_offset, y_offset, cout, want_bias)


def conv2d_strided_device(x, w, bias=None, stride=1, residual=None, act="linear", alpha=0.2, out=None, out_offset=0):
    """A 'same' float32 convolution of stride 1 or 2 with many output channels and an optional residual add, in the fixed
    summation order of include/dtfill.h, dtfill_conv2d_strided (a layer of net.py's ResNet18_NO_BN_l2).  x: contiguous float32
    CUDA tensor [B,H,W,Cin]; w: [ksize,ksize,Cin,Cout], a Keras Conv2D.kernel as stored; Cin and Cout multiples of 16; bias:
    [Cout] or None; residual: contiguous [B,Ho,Wo,Cout] or None, added after the bias and before the activation (it may be x,
    not out); Ho = ceil(H / stride), Wo likewise, TensorFlow's 'same' rule.  out: a contiguous float32 tensor [B,Ho,Wo,C] of
    which the channels out_offset .. out_offset + Cout - 1 are written; a new [B,Ho,Wo,Cout] tensor by default.  Returns out.
    Asynchronous on the current stream; the shapes the library takes are the header's (DtfillError otherwise)."""
    return _forward("strided", x, w, bias, stride, residual, act, alpha, out, out_offset)


def conv2d_transpose_device(x, w_packed, bias=None, act="linear", alpha=0.2, out=None, out_offset=0):
    """tf.keras.layers.Conv2DTranspose(Cout, 3, strides=2, padding='same') in the fixed summation order of include/dtfill.h,
    dtfill_conv2d_transpose.  x: contiguous float32 CUDA tensor [B,H,W,Cin]; w_packed: [3,3,Cin,Cout], pack_transpose_kernel()
    of the layer's kernel; bias: [Cout] or None.  out: [B,2H,2W,C], written at out_offset .. out_offset + Cout - 1; a new
    [B,2H,2W,Cout] tensor by default.  Returns out.  Asynchronous on the current stream."""
    return _forward("transposed", x, w_packed, bias, 2, None, act, alpha, out, out_offset)


def conv2d_wide_backward_workspace_bytes(B, H, W, Cin, ksize, Cout, stride=1, transposed=False):
    """The bytes of workspace either backward call of a wide layer needs (dtfill_conv2d_wide_backward_workspace_bytes): host
    arithmetic, no device.  B, H, W, Cin: the forward's input shape.  DtfillError for a shape outside the domain."""
    return _device._sized(_lib.load().dtfill_conv2d_wide_backward_workspace_bytes(int(B), int(H), int(W), int(Cin), int(ksize),
                                                                                 int(Cout), int(stride), int(bool(transposed))))


def conv2d_strided_backward_data_device(dy, w, stride=1, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0, dx=None,
                                        dx_offset=0, want_residual=False):
    """The gradient of conv2d_strided_device with respect to x, and with want_residual to its residual, in the fixed order of
    include/dtfill.h, dtfill_conv2d_strided_backward_data.  dy: contiguous float32 CUDA tensor [B,Ho,Wo,C], the gradient of the
    layer's output in the channels dy_offset .. dy_offset + Cout - 1; w: the layer's [ksize,ksize,Cin,Cout]; y: the forward's
    output, read at y_offset likewise, needed unless act is "linear".  The forward's input frame is [stride Ho, stride Wo]: at
    stride 2 only even frames have a backward.  dx: a contiguous float32 tensor [B,H,W,C'] written at dx_offset .. dx_offset +
    Cin - 1; a new [B,H,W,Cin] tensor by default.  Returns dx, or (dx, dresidual [B,Ho,Wo,Cout]) with want_residual.
    Asynchronous on the current stream."""
    return _backward_data("strided", dy, w, stride, y, act, alpha, dy_offset, y_offset, dx, dx_offset, want_residual)


def conv2d_strided_backward_weights_device(x, dy, ksize, stride=1, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0, cout=None,
                                           want_bias=True):
    """The gradients of conv2d_strided_device with respect to w and bias, in the fixed two-level order of include/dtfill.h,
    dtfill_conv2d_strided_backward_weights.  x: the forward's input [B,H,W,Cin] (H and W even at stride 2); dy [B,H / stride,
    W / stride,C], y, act, alpha and the offsets as in conv2d_strided_backward_data_device; cout: the layer's output channels
    (default: all of dy's).  Returns (dw [ksize,ksize,Cin,Cout], db [Cout] or None without want_bias): new tensors.
    Asynchronous on the current stream."""
    return _backward_weights("strided", x, dy, ksize, stride, y, act, alpha, dy_offset, y_offset, cout, want_bias)


def conv2d_transpose_backward_data_device(dy, w_packed, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0, dx=None, dx_offset=0):
    """The gradient of conv2d_transpose_device with respect to x, in the fixed order of include/dtfill.h,
    dtfill_conv2d_transpose_backward_data.  dy: [B,2H,2W,C], read at dy_offset; w_packed: the [3,3,Cin,Cout] the forward takes;
    y: the forward's output, needed unless act is "linear".  dx: [B,H,W,C'], written at dx_offset .. dx_offset + Cin - 1; a
    new [B,H,W,Cin] tensor by default.  Returns dx.  Asynchronous on the current stream."""
    return _backward_data("transposed", dy, w_packed, 2, y, act, alpha, dy_offset, y_offset, dx, dx_offset)


def conv2d_transpose_backward_weights_device(x, dy, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0, cout=None, want_bias=True):
    """The gradients of conv2d_transpose_device with respect to w_packed and bias, in the fixed two-level order of
    include/dtfill.h, dtfill_conv2d_transpose_backward_weights.  x: the forward's input [B,H,W,Cin]; dy [B,2H,2W,C].  Returns
    (dw in the packed layout [3,3,Cin,Cout], db [Cout] or None without want_bias): new tensors; the gradient of the Keras kernel
    [3,3,Cout,Cin] is dw.permute(0, 1, 3, 2).  Asynchronous on the current stream."""
    return _backward_weights("transposed", x, dy, 3, 2, y, act, alpha, dy_offset, y_offset, cout, want_bias)


def conv2d_image_device(x, w, bias=None, act="linear", alpha=0.2, out=None, out_offset=0):
    """A stride-1 'same' float32 convolution of an image of 2, 3 or 4 channels into a multiple of 16 channels, in the fixed
    summation order of include/dtfill.h, dtfill_conv2d_image (img_conv of net.py's ResNet18_NO_BN_l2_image).  x: contiguous
    float32 CUDA tensor [B,H,W,Cin], what rgb_read_device emits; w: [ksize,ksize,Cin,Cout], a Keras Conv2D.kernel as stored;
    bias: [Cout] or None; act, alpha, out and out_offset as in conv2d_device.  Returns out.  Asynchronous on the current stream;
    the shapes the library takes are the header's (DtfillError otherwise)."""
    return _forward("image", x, w, bias, 1, None, act, alpha, out, out_offset)


def conv2d_image_backward_workspace_bytes(B, H, W, Cin, ksize, Cout):
    """The bytes of workspace conv2d_image_backward_weights_device needs (dtfill_conv2d_image_backward_workspace_bytes): host
    arithmetic, no device.  DtfillError for a shape outside dtfill_conv2d_image's domain."""
    return _device._sized(_lib.load().dtfill_conv2d_image_backward_workspace_bytes(int(B), int(H), int(W), int(Cin), int(ksize),
                                                                                  int(Cout)))


def conv2d_image_backward_weights_device(x, dy, ksize, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0, cout=None,
                                         want_bias=True):
    """The gradients of conv2d_image_device with respect to w and bias, in the fixed two-level order of include/dtfill.h,
    dtfill_conv2d_image_backward_weights.  x: the forward's input [B,H,W,Cin]; dy, y, act, alpha, the offsets and cout as in
    conv2d_backward_weights_device.  Returns (dw [ksize,ksize,Cin,Cout], db [Cout] or None without want_bias): new tensors.
    There is no data gradient: the image is data.  Asynchronous on the current stream."""
    return _backward_weights("image", x, dy, ksize, 1, y, act, alpha, dy_offset, y_offset, cout, want_bias)


def pack_bf16_device(w, transposed=False):
    """The packed bf16 weights the bf16 convolutions take, made on the device by dtfill_conv2d_pack_bf16.  w: contiguous float32
    CUDA tensor in the form the float32 function takes: [ksize,ksize,Cin,Cout] with ksize 1 or 3, and with transposed the
    already exchanged [3,3,Cin,Cout] (pack_transpose_kernel).  Returns a new bfloat16 tensor [ksize,ksize,G,Cout / 16,64,8],
    G = ceil(Cin / 32): the matrix cores' B fragments, rounded to nearest even, half groups zero-filled.  The layout is the
    header's and opaque: hand the tensor to conv2d_strided_bf16_device or conv2d_transpose_bf16_device and nothing else.
    Asynchronous on the current stream."""
    _require_gpu()
    _check_tensor(w, "w", layout="[3,3,Cin,Cout]" if transposed else "[ksize,ksize,Cin,Cout]")
    ksize, Cin, Cout = w.shape[0], w.shape[2], w.shape[3]
    if w.shape[1] != ksize or (transposed and ksize != 3):
        raise ValueError("w must be %s, got %s" % ("[3,3,Cin,Cout]" if transposed else "[ksize,ksize,Cin,Cout]", tuple(w.shape)))
    L = _lib.load()
    elems = _device._sized(L.dtfill_conv2d_bf16_packed_elems(ksize, Cin, Cout))
    packed = torch.empty((ksize, ksize, elems // (ksize * ksize * (Cout // 16) * 512), Cout // 16, 64, 8), dtype=torch.bfloat16,
                         device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(L.dtfill_conv2d_pack_bf16(w.data_ptr(), ksize, Cin, Cout, packed.data_ptr(), _stream(w.device)))
    return packed


def _forward_bf16(kind, x, packed, bias, stride, residual, act, alpha, out, out_offset):
    """The forward of a wide layer of `kind` on the bf16 matrix cores: _forward's sequence over the packed weights, whose
    shape [ksize,ksize,G,Cout / 16,64,8] says the layer's ksize and Cout; Cin is x's."""
    k = _KINDS[kind]
    if stride not in (1, 2):
        raise ValueError("stride must be 1 or 2, got %r" % (stride,))
    _check_act(act)
    _check_tensor(x, "x", layout="[B,H,W,Cin]")
    B, H, W, Cin = x.shape
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.bfloat16 or packed.dim() != 6 or not packed.is_contiguous():
        raise ValueError("w_packed must be what pack_bf16_device returns, a contiguous bfloat16 tensor of six axes")
    ksize, Cout = packed.shape[0], 16 * packed.shape[3]
    if (tuple(packed.shape[1:3]) + tuple(packed.shape[4:]) != (ksize, -(-Cin // 32), 64, 8) or ksize != (k.ksize or ksize)
            or packed.device != x.device):
        raise ValueError("w_packed must be pack_bf16_device's of a %s kernel with Cin = %d on %s, got %s"
                         % (k.w_layout, Cin, x.device, tuple(packed.shape)))
    if bias is not None:
        _check_tensor(bias, "bias", layout="[Cout]")
        if bias.shape[0] != Cout or bias.device != x.device:
            raise ValueError("bias must be [%d] on %s, got %s" % (Cout, x.device, tuple(bias.shape)))
    out = _check_frames(kind, x, Cout, stride, residual, out, out_offset)
    with torch.cuda.device(x.device):
        _lib.check(getattr(_lib.load(), k.forward + "_bf16")(
            x.data_ptr(), B, H, W, Cin, packed.data_ptr(), _ptr(bias), *k.abi_shape(ksize, Cout, stride),
            *((_ptr(residual),) if k.has_residual else ()), _lib.CONV_ACTS[act], float(alpha), out.data_ptr(), out.shape[3],
            int(out_offset), _stream(x.device)))
    return out


def conv2d_strided_bf16_device(x, w_packed, bias=None, stride=1, residual=None, act="linear", alpha=0.2, out=None, out_offset=0):
    """conv2d_strided_device on the bf16 matrix cores with float32 accumulation (include/dtfill.h, dtfill_conv2d_strided_bf16):
    x, bias, residual and out are the float32 tensors of conv2d_strided_device, w_packed is pack_bf16_device(w) of its w, ksize
    1 or 3.  The operands are rounded to bf16 (to nearest even), the sum and the finish are float32; the result lies within the
    header's bound of the exact sum and its bits are a function of the inputs and the shape alone.  Returns out.  Asynchronous
    on the current stream."""
    return _forward_bf16("strided", x, w_packed, bias, stride, residual, act, alpha, out, out_offset)


def conv2d_transpose_bf16_device(x, w_packed, bias=None, act="linear", alpha=0.2, out=None, out_offset=0):
    """conv2d_transpose_device on the bf16 matrix cores with float32 accumulation (dtfill_conv2d_transpose_bf16): w_packed is
    pack_bf16_device(w, transposed=True) of the [3,3,Cin,Cout] kernel conv2d_transpose_device takes.  Everything else as
    conv2d_strided_bf16_device.  Returns out, [B,2H,2W,C].  Asynchronous on the current stream."""
    return _forward_bf16("transposed", x, w_packed, bias, 2, None, act, alpha, out, out_offset)


def conv2d_strided_bf16(x, kernel, bias=None, stride=1, residual=None, act="linear", alpha=0.2):
    """conv2d_strided_bf16_device as a numpy function: the arguments of conv2d_strided, the kernel packed here.  Returns
    float32 [B,Ho,Wo,Cout]."""
    a, k, b, r = _uploaded(x, kernel, bias, residual)
    return conv2d_strided_bf16_device(a, pack_bf16_device(k), b, stride, r, act, alpha).cpu().numpy()


def conv2d_transpose_bf16(x, kernel, bias=None, act="linear", alpha=0.2):
    """conv2d_transpose_bf16_device as a numpy function: the arguments of conv2d_transpose, kernel [3,3,Cout,Cin] as Keras
    stores a Conv2DTranspose's (exchanged and packed here).  Returns float32 [B,2H,2W,Cout]."""
    a, k, b = _uploaded(x, kernel, bias)
    return conv2d_transpose_bf16_device(a, pack_bf16_device(k.permute(0, 1, 3, 2).contiguous(), transposed=True), b, act, alpha).cpu().numpy()


def conv2d_wide_backward_bf16_workspace_bytes(B, H, W, Cin, ksize, Cout, stride=1, transposed=False):
    """The bytes of workspace either bf16 backward call of a wide layer needs (dtfill_conv2d_wide_backward_bf16_workspace_bytes):
    host arithmetic, no device.  DtfillError for a shape outside the domain (ksize 1 or 3)."""
    return _device._sized(_lib.load().dtfill_conv2d_wide_backward_bf16_workspace_bytes(int(B), int(H), int(W), int(Cin), int(ksize),
                                                                                      int(Cout), int(stride), int(bool(transposed))))


def conv2d_strided_backward_data_bf16_device(dy, w, stride=1, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0, dx=None,
                                             dx_offset=0, want_residual=False):
    """conv2d_strided_backward_data_device on the bf16 matrix cores with float32 accumulation (include/dtfill.h,
    dtfill_conv2d_strided_backward_data_bf16): the same float32 tensors, w the plain float32 [ksize,ksize,Cin,Cout] with ksize
    1 or 3 (packed inside the call).  g = dy act'(y) is made in float32 and dresidual is g exactly; dx is the bf16 forward over
    g under the flipped or exchanged kernel, bit for bit, within the header's bound.  Asynchronous on the current stream."""
    return _backward_data("strided", dy, w, stride, y, act, alpha, dy_offset, y_offset, dx, dx_offset, want_residual, "bf16")


def conv2d_strided_backward_weights_bf16_device(x, dy, ksize, stride=1, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0,
                                                cout=None, want_bias=True):
    """conv2d_strided_backward_weights_device on the bf16 matrix cores with float32 accumulation
    (dtfill_conv2d_strided_backward_weights_bf16): x and g rounded to bf16 in registers, one MFMA per 32 pixels, tap and tile
    into float32 partials per segment, the segments added in float32 in a fixed order.  The bits are a function of the inputs
    and the shape alone and lie within the header's bound of the exact sum.  Returns (dw, db or None): new float32 tensors."""
    return _backward_weights("strided", x, dy, ksize, stride, y, act, alpha, dy_offset, y_offset, cout, want_bias, "bf16")


def conv2d_transpose_backward_data_bf16_device(dy, w_packed, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0, dx=None,
                                               dx_offset=0):
    """conv2d_transpose_backward_data_device on the bf16 matrix cores (dtfill_conv2d_transpose_backward_data_bf16): w_packed is
    the float32 [3,3,Cin,Cout] that function takes.  Everything else as conv2d_strided_backward_data_bf16_device."""
    return _backward_data("transposed", dy, w_packed, 2, y, act, alpha, dy_offset, y_offset, dx, dx_offset, False, "bf16")


def conv2d_transpose_backward_weights_bf16_device(x, dy, y=None, act="linear", alpha=0.2, dy_offset=0, y_offset=0, cout=None,
                                                  want_bias=True):
    """conv2d_transpose_backward_weights_device on the bf16 matrix cores (dtfill_conv2d_transpose_backward_weights_bf16).
    Returns (dw in the packed layout [3,3,Cin,Cout], db or None).  As conv2d_strided_backward_weights_bf16_device."""
    return _backward_weights("transposed", x, dy, 3, 2, y, act, alpha, dy_offset, y_offset, cout, want_bias, "bf16")


def _numpy_or_none(t):
    return None if t is None else t.cpu().numpy()


def conv2d_strided_backward_data_bf16(dy, kernel, stride=1, y=None, act="linear", alpha=0.2, want_residual=False):
    """conv2d_strided_backward_data_bf16_device as a numpy function: dy [B,Ho,Wo,Cout], kernel [ksize,ksize,Cin,Cout], y like dy
    or None.  Returns float32 dx [B,stride Ho,stride Wo,Cin], or (dx, dresidual) with want_residual."""
    d, k, yy = _uploaded(dy, kernel, y)
    out = conv2d_strided_backward_data_bf16_device(d, k, stride, yy, act, alpha, want_residual=want_residual)
    return tuple(t.cpu().numpy() for t in out) if want_residual else out.cpu().numpy()


def conv2d_strided_backward_weights_bf16(x, dy, ksize, stride=1, y=None, act="linear", alpha=0.2, want_bias=True):
    """conv2d_strided_backward_weights_bf16_device as a numpy function.  Returns float32 (dw [ksize,ksize,Cin,Cout], db [Cout] or
    None)."""
    a, d, yy = _uploaded(x, dy, y)
    return tuple(_numpy_or_none(t) for t in conv2d_strided_backward_weights_bf16_device(a, d, ksize, stride, yy, act, alpha,
                                                                                       want_bias=want_bias))


def conv2d_transpose_backward_data_bf16(dy, kernel, y=None, act="linear", alpha=0.2):
    """conv2d_transpose_backward_data_bf16_device as a numpy function: dy [B,2H,2W,Cout], kernel [3,3,Cout,Cin] as Keras stores a
    Conv2DTranspose's (exchanged here).  Returns float32 dx [B,H,W,Cin]."""
    d, k, yy = _uploaded(dy, kernel, y)
    return conv2d_transpose_backward_data_bf16_device(d, k.permute(0, 1, 3, 2).contiguous(), yy, act, alpha).cpu().numpy()


def conv2d_transpose_backward_weights_bf16(x, dy, y=None, act="linear", alpha=0.2, want_bias=True):
    """conv2d_transpose_backward_weights_bf16_device as a numpy function.  Returns float32 (dw [3,3,Cout,Cin] in Keras' layout, db
    [Cout] or None)."""
    a, d, yy = _uploaded(x, dy, y)
    dw, db = conv2d_transpose_backward_weights_bf16_device(a, d, yy, act, alpha, want_bias=want_bias)
    return dw.permute(0, 1, 3, 2).contiguous().cpu().numpy(), _numpy_or_none(db)


def pack_transpose_kernel(kernel):
    """A Keras Conv2DTranspose.kernel [3,3,Cout,Cin] -> the ABI's [3,3,Cin,Cout], contiguous float32: the last two axes
    exchanged, once, when the weights are loaded."""
    k = np.asarray(kernel, dtype=np.float32)
    if k.ndim != 4 or k.shape[:2] != (3, 3):
        raise ValueError("a Conv2DTranspose kernel is [3,3,Cout,Cin], got %s" % (k.shape,))
    return np.ascontiguousarray(k.transpose(0, 1, 3, 2))


def _uploaded(x, kernel, *others):
    """Host arrays of a numpy form, checked as tools.conv2d checks its own, as tensors on the default operator's device (None
    stays None)."""
    from .tools import _as_f32_frames, _upload

    arrays = [None if a is None else _as_f32_frames(a) for a in (x, kernel) + others]
    if arrays[0].ndim != 4 or arrays[1].ndim != 4:
        raise ValueError("expected x [B,H,W,Cin] and a kernel of four axes")
    dev = _device.default_op().device
    return [None if a is None else _upload(a, dev) for a in arrays]


def conv2d_strided(x, kernel, bias=None, stride=1, residual=None, act="linear", alpha=0.2):
    """conv2d_strided_device as a numpy function: x [B,H,W,Cin], kernel [ksize,ksize,Cin,Cout] and bias [Cout] as Keras stores
    them, residual [B,Ho,Wo,Cout] or None.  Returns float32 [B,Ho,Wo,Cout]."""
    a, k, b, r = _uploaded(x, kernel, bias, residual)
    return conv2d_strided_device(a, k, b, stride, r, act, alpha).cpu().numpy()


def conv2d_transpose(x, kernel, bias=None, act="linear", alpha=0.2):
    """conv2d_transpose_device as a numpy function: x [B,H,W,Cin], kernel [3,3,Cout,Cin] as Keras stores a Conv2DTranspose's
    (packed here), bias [Cout].  Returns float32 [B,2H,2W,Cout]."""
    a, k, b = _uploaded(x, kernel, bias)
    return conv2d_transpose_device(a, k.permute(0, 1, 3, 2).contiguous(), b, act, alpha).cpu().numpy()


def conv2d_image(x, kernel, bias=None, act="linear", alpha=0.2):
    """conv2d_image_device as a numpy function: x [B,H,W,Cin] with Cin 2, 3 or 4, kernel [ksize,ksize,Cin,Cout] and bias [Cout]
    as Keras stores them.  Returns float32 [B,H,W,Cout]."""
    a, k, b = _uploaded(x, kernel, bias)
    return conv2d_image_device(a, k, b, act, alpha).cpu().numpy()
