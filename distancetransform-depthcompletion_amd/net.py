"""The reference's networks as inference classes on the device: SparsityCNN (solution_DeepNet/net.py:11-242), its light
network, and ResNet18 (ResNet18_NO_BN_l2, net.py:245-745), the paper's.  Every convolution is a fixed-order float32 chain of
include/dtfill.h (dtfill_conv2d, dtfill_conv2d_strided, dtfill_conv2d_transpose), the multi-channel fill in the middle is
dtfill_generate_multi_channel, and the elementwise steps are single IEEE operations in torch.  So the output bits are a
function of the weights and the input alone, from run to run and from shape to shape.  SparsityCNNTrainable is SparsityCNN
under a tape, a torch.nn.Module over autograd.conv2d, for train.py:232-254's step; conv2d_backward_data_device and
conv2d_backward_weights_device are the device functions of one layer's backward (dtfill_conv2d_backward_data, _weights).
ResNet18Trainable is ResNet18 under a tape, over autograd.conv2d_strided and autograd.conv2d_transpose, the network train.py:113
trains; conv2d_strided_backward_data_device, conv2d_strided_backward_weights_device, conv2d_transpose_backward_data_device and
conv2d_transpose_backward_weights_device are the device functions of a wide layer's backward.  The six are one path: each is
a call of _backward_data or _backward_weights, which hold the checks, the frames, the outputs, the workspace and the ABI call
once, under a kind (narrow, strided, transposed) whose entry in _KINDS supplies the frame arithmetic, the symbol and the
arguments only that kind takes.

ResNet18Image and ResNet18ImageTrainable are ResNet18_NO_BN_l2_image (net.py:3383-3893), the image-guided network demo.py
defaults to: ResNet18 with img_conv, the layer that reads the [B,H,W,3] image (dtfill_conv2d_image, conv2d_image_device, and
conv2d_image_backward_weights_device, a fourth kind with no data gradient), in front of the stems.

ResNet18LightImage and ResNet18LightImageTrainable are ResNet18_NO_BN_l2_light_image (net.py:3895-4426), the image-guided network
at 64 channels on every level.  Its call() pools conv1_pre's output by 2, 4 and 8 (tf.nn.max_pool, net.py:4285, 4320, 4353):
that is ONE dtfill_max_pool_pyramid call here (device.max_pool_pyramid_device, autograd.max_pool_pyramid).

The other eight models of the reference's net.py are not here.  ResNet18_NO_BN_l2_large_image lacks only its own trunk wiring: it
has no pooling and no stride-4 or stride-8 layer (those are commented-out lines of the reference), so its layers are all here.
conv2d_device, conv2d_strided_device and conv2d_transpose_device, the device
functions of one convolution, are reached as device.<name> as well; they live here, beside device.py's helpers, with their
argument checks in tests/test_conv2d.py, tests/test_gpu_conv2d.py, tests/test_conv2d_strided.py and
tests/test_gpu_conv2d_strided.py.
"""
import collections

import numpy as np
import torch

from . import _lib
from . import device as _device
from .device import _check_tensor, _ptr, _require_gpu, _stream

LEAKY_ALPHA = 0.2  # tf.nn.leaky_relu's default
STEM_WIDTH = 16  # channels every stem writes of the [B,H,W,16 * scale_num] tensor conv1a reads


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


def conv2d_device(x, w, bias=None, act="linear", alpha=0.2, out=None, out_offset=0):
    """A stride-1 'same' float32 convolution in the fixed summation order of include/dtfill.h, dtfill_conv2d (a layer of
    net.py's SparsityCNN).  x: contiguous float32 CUDA tensor [B,H,W,Cin], or [B,H,W] for Cin = 1; w: [ksize,ksize,Cin,Cout], a
    Keras Conv2D.kernel as stored (cross-correlation); bias: [Cout] or None; act: "linear" or "leaky" (y > 0 ? y : y * alpha).
    out: a contiguous float32 tensor [B,H,W,C] on x's device of which the channels out_offset .. out_offset + Cout - 1 are
    written and the others left as they are (not x itself); a new [B,H,W,Cout] tensor by default.  Returns out.  Asynchronous on
    the current stream; the shapes the library takes are the header's (DtfillError otherwise)."""
    B, H, W, Cin, Cout = _check_conv_args(x, w, bias, act, "[ksize,ksize,Cin,Cout]", plane_ok=True)
    out = _check_conv_out(x, out, out_offset, (B, H, W), Cout)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dtfill_conv2d(x.data_ptr(), B, H, W, Cin, w.data_ptr(), _ptr(bias), w.shape[0], Cout,
                                             _lib.CONV_ACTS[act], float(alpha), out.data_ptr(), out.shape[3], int(out_offset),
                                             _stream(x.device)))
    return out


_convb_ws = _device._Scratch()  # the workspace of the backward calls, of every kind of layer


def conv2d_backward_workspace_bytes(B, H, W, Cin, ksize, Cout):
    """The bytes of workspace either backward call of a layer needs (dtfill_conv2d_backward_workspace_bytes): host arithmetic,
    no device.  DtfillError for a shape outside dtfill_conv2d's domain."""
    return _device._sized(_lib.load().dtfill_conv2d_backward_workspace_bytes(int(B), int(H), int(W), int(Cin), int(ksize), int(Cout)))


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


# What tells the four kinds of layer apart in the backward.  data, weights: the ABI's symbols (data None: the image layer has
# no data gradient); abi_shape(ksize, Cout, stride):
# what they take between Cin and act; has_residual: the data call takes dresidual; ws_bytes(L, B, H, W, Cin, ksize, Cout,
# stride): the library's size function; ksize: the [3,3,..] rule, or None for any square kernel; x_frame(Ho, Wo, stride): the
# forward's input frame under a dy of [Ho,Wo], and dy_frame(H, W, stride) the reverse, each None where the kind has no such
# layer (the evenness rule).
_Kind = collections.namedtuple("_Kind", "data weights abi_shape has_residual ws_bytes w_name w_layout ksize dy_layout plane_ok "
                                        "x_frame dy_frame")
_KINDS = {
    "narrow": _Kind("dtfill_conv2d_backward_data", "dtfill_conv2d_backward_weights", lambda ksize, Cout, s: (ksize, Cout), False,
                    lambda L, B, H, W, Cin, ksize, Cout, s: L.dtfill_conv2d_backward_workspace_bytes(B, H, W, Cin, ksize, Cout),
                    "w", "[ksize,ksize,Cin,Cout]", None, "[B,H,W,C]", True, lambda Ho, Wo, s: (Ho, Wo), lambda H, W, s: (H, W)),
    "strided": _Kind("dtfill_conv2d_strided_backward_data", "dtfill_conv2d_strided_backward_weights",
                     lambda ksize, Cout, s: (ksize, Cout, s), True,
                     lambda L, B, H, W, Cin, ksize, Cout, s: L.dtfill_conv2d_wide_backward_workspace_bytes(B, H, W, Cin, ksize, Cout, s, 0),
                     "w", "[ksize,ksize,Cin,Cout]", None, "[B,Ho,Wo,C]", False, lambda Ho, Wo, s: (s * Ho, s * Wo),
                     lambda H, W, s: None if H % s or W % s else (H // s, W // s)),
    "transposed": _Kind("dtfill_conv2d_transpose_backward_data", "dtfill_conv2d_transpose_backward_weights",
                        lambda ksize, Cout, s: (Cout,), False,
                        lambda L, B, H, W, Cin, ksize, Cout, s: L.dtfill_conv2d_wide_backward_workspace_bytes(B, H, W, Cin, 3, Cout, 2, 1),
                        "w_packed", "[3,3,Cin,Cout]", 3, "[B,2H,2W,C]", False,
                        lambda Ho, Wo, s: None if Ho % 2 or Wo % 2 else (Ho // 2, Wo // 2), lambda H, W, s: (2 * H, 2 * W)),
    # the layer that reads the image: no data call, the image is data
    "image": _Kind(None, "dtfill_conv2d_image_backward_weights", lambda ksize, Cout, s: (ksize, Cout), False,
                   lambda L, B, H, W, Cin, ksize, Cout, s: L.dtfill_conv2d_image_backward_workspace_bytes(B, H, W, Cin, ksize, Cout),
                   "w", "[ksize,ksize,Cin,Cout]", None, "[B,H,W,C]", False, lambda Ho, Wo, s: (Ho, Wo), lambda H, W, s: (H, W)),
}


def _check_backward_kind(kind, act, alpha, stride):
    _check_act(act, alpha)
    if stride not in (1, 2):
        raise ValueError("stride must be 1 or 2, got %r" % (stride,))
    return _KINDS[kind]


def _backward_data(kind, dy, w, stride, y, act, alpha, dy_offset, y_offset, dx, dx_offset, want_residual=False):
    """The data gradient of a layer of `kind`: the six public functions' shared sequence, once."""
    k = _check_backward_kind(kind, act, alpha, stride)
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
    nbytes = _device._sized(k.ws_bytes(L, B, H, W, Cin, ksize, Cout, stride))
    with torch.cuda.device(dy.device):
        with _convb_ws.hold(dy.device, nbytes) as ws:
            _lib.check(getattr(L, k.data)(
                dy.data_ptr(), Cdy, int(dy_offset), _ptr(y), Cy, int(y_offset), w.data_ptr(), B, H, W, Cin,
                *k.abi_shape(ksize, Cout, stride), _lib.CONV_ACTS[act], float(alpha), dx.data_ptr(), dx.shape[3], int(dx_offset),
                *((_ptr(dres),) if k.has_residual else ()), ws, nbytes, _stream(dy.device)))
    return (dx, dres) if want_residual else dx


def _backward_weights(kind, x, dy, ksize, stride, y, act, alpha, dy_offset, y_offset, cout, want_bias):
    """The weight and bias gradients of a layer of `kind`: the shared sequence, once."""
    k = _check_backward_kind(kind, act, alpha, stride)
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
    nbytes = _device._sized(k.ws_bytes(L, B, H, W, Cin, ksize, Cout, stride))
    dw = torch.empty((ksize, ksize, Cin, Cout), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if want_bias else None
    with torch.cuda.device(x.device):
        with _convb_ws.hold(x.device, nbytes) as ws:
            _lib.check(getattr(L, k.weights)(
                x.data_ptr(), dy.data_ptr(), Cdy, int(dy_offset), _ptr(y), Cy, int(y_offset), B, H, W, Cin,
                *k.abi_shape(ksize, Cout, stride), _lib.CONV_ACTS[act], float(alpha), dw.data_ptr(), _ptr(db), ws, nbytes,
                _stream(x.device)))
    return dw, db


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
    if stride not in (1, 2):
        raise ValueError("stride must be 1 or 2, got %r" % (stride,))
    B, H, W, Cin, Cout = _check_conv_args(x, w, bias, act, "[ksize,ksize,Cin,Cout]")
    frame = (B, -(-H // stride), -(-W // stride))
    if residual is not None:
        _check_tensor(residual, "residual", layout="[B,Ho,Wo,Cout]")
        if tuple(residual.shape) != frame + (Cout,) or residual.device != x.device:
            raise ValueError("residual must be %s on %s, got %s" % (frame + (Cout,), x.device, tuple(residual.shape)))
    out = _check_conv_out(x, out, out_offset, frame, Cout)
    if residual is not None and out.data_ptr() == residual.data_ptr():
        raise ValueError("out may not alias residual")
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dtfill_conv2d_strided(x.data_ptr(), B, H, W, Cin, w.data_ptr(), _ptr(bias), w.shape[0], Cout,
                                                     stride, _ptr(residual), _lib.CONV_ACTS[act], float(alpha), out.data_ptr(),
                                                     out.shape[3], int(out_offset), _stream(x.device)))
    return out


def conv2d_transpose_device(x, w_packed, bias=None, act="linear", alpha=0.2, out=None, out_offset=0):
    """tf.keras.layers.Conv2DTranspose(Cout, 3, strides=2, padding='same') in the fixed summation order of include/dtfill.h,
    dtfill_conv2d_transpose.  x: contiguous float32 CUDA tensor [B,H,W,Cin]; w_packed: [3,3,Cin,Cout], pack_transpose_kernel()
    of the layer's kernel; bias: [Cout] or None.  out: [B,2H,2W,C], written at out_offset .. out_offset + Cout - 1; a new
    [B,2H,2W,Cout] tensor by default.  Returns out.  Asynchronous on the current stream."""
    B, H, W, Cin, Cout = _check_conv_args(x, w_packed, bias, act, "[3,3,Cin,Cout]")
    if w_packed.shape[0] != 3:
        raise ValueError("w_packed must be [3,3,Cin,Cout], got %s" % (tuple(w_packed.shape),))
    out = _check_conv_out(x, out, out_offset, (B, 2 * H, 2 * W), Cout)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dtfill_conv2d_transpose(x.data_ptr(), B, H, W, Cin, w_packed.data_ptr(), _ptr(bias), Cout,
                                                       _lib.CONV_ACTS[act], float(alpha), out.data_ptr(), out.shape[3],
                                                       int(out_offset), _stream(x.device)))
    return out


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
    B, H, W, Cin, Cout = _check_conv_args(x, w, bias, act, "[ksize,ksize,Cin,Cout]")
    out = _check_conv_out(x, out, out_offset, (B, H, W), Cout)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dtfill_conv2d_image(x.data_ptr(), B, H, W, Cin, w.data_ptr(), _ptr(bias), w.shape[0], Cout,
                                                   _lib.CONV_ACTS[act], float(alpha), out.data_ptr(), out.shape[3],
                                                   int(out_offset), _stream(x.device)))
    return out


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


def stem_layers(scale_num):
    """The layer that reads lidar_1 .. lidar_<scale_num>, in that order.  net.py:206 calls lidar_conv_extra_1 again on
    lidar_4: lidar_conv_extra_3 is built (net.py:46) and never used, and that is reproduced here."""
    if scale_num not in (1, 2, 3, 4):
        raise ValueError("scale_num must be 1, 2, 3 or 4, got %r" % (scale_num,))
    return ("lidar_conv", "lidar_conv_extra_1", "lidar_conv_extra_2", "lidar_conv_extra_1")[:scale_num]


def _head_shapes(scale_num, if_correct):
    """The layers of the head the two networks share: the correction branch and the stems."""
    shapes = {}
    if if_correct:
        shapes.update(correct_1=(7, 1, 16), correct_2=(5, 16, 16), correct_3=(3, 16, 16), correct_4=(3, 16, 1))
    for name in stem_layers(scale_num):
        shapes[name] = (3, 1, STEM_WIDTH)
    return shapes


def layer_shapes(scale_num=4, if_correct=True):
    """{layer name: (ksize, Cin, Cout)} of the layers the forward uses, under the reference's attribute names."""
    shapes = _head_shapes(scale_num, if_correct)
    shapes.update(conv1a=(7, STEM_WIDTH * scale_num, 16), conv1b=(5, 16, 16), conv1c=(3, 16, 16), conv1d=(3, 16, 16),
                  conv_output=(1, 16, 1))
    return shapes


_KNOWN = tuple(layer_shapes(4, True)) + ("lidar_conv_extra_3",)  # every attribute name of the reference's class


def _glorot(shapes_of, seed, scale_num, if_correct, bias):
    rng = np.random.default_rng(seed)
    shapes = shapes_of(scale_num, if_correct)
    if scale_num > 3:
        shapes["lidar_conv_extra_3"] = (3, 1, STEM_WIDTH)
    weights = {}
    for name, (k, cin, cout) in shapes.items():
        limit = np.sqrt(6.0 / (k * k * (cin + cout)))
        weights[name] = (rng.uniform(-limit, limit, _keras_shape(name, k, cin, cout)).astype(np.float32),
                         rng.uniform(-bias, bias, (cout,)).astype(np.float32))
    return weights


def glorot_weights(seed, scale_num=4, if_correct=True, bias=0.0):
    """A weights dict for tests and benchmarks: Keras' default glorot_uniform kernels, uniform(+-sqrt(6 / (fan_in + fan_out))),
    and biases uniform in +-bias (Keras starts them at zero), as float32 numpy arrays of Keras' shapes.  Holds
    lidar_conv_extra_3 when the reference would build it (scale_num 4)."""
    return _glorot(layer_shapes, seed, scale_num, if_correct, bias)


RESNET_WIDTHS = (64, 128, 256, 512)  # channels of levels 1 .. 4; level k lives at 1 / 2^(k-1) of the frame each way
RESNET_STRIDE2 = ("conv2a", "conv2a_extra", "conv3a", "conv3a_extra", "conv4a", "conv4a_extra")
RESNET_TRANSPOSED = ("upsample_4", "upsample_3", "upsample_2")  # Conv2DTranspose: Keras stores [3,3,Cout,Cin]


def layer_shapes_resnet18(scale_num=4, if_correct=True):
    """{layer name: (ksize, Cin, Cout)} of the layers ResNet18_NO_BN_l2's forward uses (net.py:262-400), under the reference's
    attribute names.  The layers of RESNET_STRIDE2 have stride 2; those of RESNET_TRANSPOSED are Conv2DTranspose(Cout, 3,
    strides=2), whose Keras kernel is [3,3,Cout,Cin]; upsample_1 is an ordinary convolution, as in the reference."""
    shapes = _head_shapes(scale_num, if_correct)
    below = STEM_WIDTH * scale_num
    for level, width in enumerate(RESNET_WIDTHS, 1):
        shapes["conv%da" % level] = (3, below, width)
        shapes["conv%db" % level] = (3, width, width)
        shapes["conv%da_extra" % level] = (1, below, width)
        shapes["conv%dc" % level] = (3, width, width)
        shapes["conv%dd" % level] = (3, width, width)
        below = width
    shapes.update(upsample_4=(3, 512, 256), upsample_4_post=(3, 512, 256), upsample_3=(3, 256, 128), upsample_3_post=(3, 256, 128),
                  upsample_2=(3, 128, 64), upsample_2_post=(3, 128, 64), upsample_1=(3, 64, 64),
                  upsample_1_post=(3, 64 + STEM_WIDTH * scale_num, 64), conv_output=(1, 64, 1))
    return shapes


IMAGE_WIDTH = 64  # channels img_conv writes in front of the stems: conv1a of the image network reads [image | stems]


def layer_shapes_resnet18_image(scale_num=4, if_correct=True):
    """{layer name: (ksize, Cin, Cout)} of the layers ResNet18_NO_BN_l2_image's forward uses (net.py:3383-3893): those of
    layer_shapes_resnet18 and img_conv, the layer that reads the image, whose 64 channels stand in front of the stems, so the
    three layers that read that tensor are 64 channels wider."""
    shapes = layer_shapes_resnet18(scale_num, if_correct)
    wide = IMAGE_WIDTH + STEM_WIDTH * scale_num
    shapes.update(img_conv=(3, 3, IMAGE_WIDTH), conv1a=(3, wide, 64), conv1a_extra=(1, wide, 64), upsample_1_post=(3, 64 + wide, 64))
    return shapes


LIGHT_WIDTH = 64  # channels of every level of the light network, and of conv1_pre's output, the tensor it pools
LIGHT_POOLS = (2, 4, 8)  # tf.nn.max_pool of conv1_pre's output behind levels 2, 3 and 4 (net.py:4285, 4320, 4353)


def layer_shapes_resnet18_light_image(scale_num=4, if_correct=True):
    """{layer name: (ksize, Cin, Cout)} of the layers ResNet18_NO_BN_l2_light_image's forward uses (net.py:3895-4426): 64 channels
    on every level.  conv1_pre folds the stems into 64 channels; conv1a and conv1a_extra read [image | conv1_pre]; the layers
    that read a level's tensor concatenated with a pooled conv1_pre output (conv3a, conv4a, their _extra, upsample_4) read 128
    channels, and the two _post layers whose skip tensor is such a concat read 192."""
    shapes = _head_shapes(scale_num, if_correct)
    w = LIGHT_WIDTH
    shapes.update(img_conv=(3, 3, IMAGE_WIDTH), conv1_pre=(3, STEM_WIDTH * scale_num, w))
    for level, below in enumerate((IMAGE_WIDTH + w, w, 2 * w, 2 * w), 1):
        shapes["conv%da" % level] = (3, below, w)
        shapes["conv%db" % level] = (3, w, w)
        shapes["conv%da_extra" % level] = (1, below, w)
        shapes["conv%dc" % level] = (3, w, w)
        shapes["conv%dd" % level] = (3, w, w)
    shapes.update(upsample_4=(3, 2 * w, w), upsample_4_post=(3, 3 * w, w), upsample_3=(3, w, w), upsample_3_post=(3, 3 * w, w),
                  upsample_2=(3, w, w), upsample_2_post=(3, 2 * w, w), upsample_1=(3, w, w), upsample_1_post=(3, 2 * w, w),
                  conv_output=(1, w, 1))
    return shapes


def _keras_shape(name, k, cin, cout):
    return (k, k, cout, cin) if name in RESNET_TRANSPOSED else (k, k, cin, cout)


def glorot_weights_resnet18(seed, scale_num=4, if_correct=True, bias=0.0):
    """glorot_weights() for ResNet18: float32 numpy arrays of Keras' shapes, [3,3,Cout,Cin] for the transposed layers."""
    return _glorot(layer_shapes_resnet18, seed, scale_num, if_correct, bias)


def glorot_weights_resnet18_image(seed, scale_num=4, if_correct=True, bias=0.0):
    """glorot_weights() for ResNet18Image: float32 numpy arrays of Keras' shapes, [3,3,Cout,Cin] for the transposed layers."""
    return _glorot(layer_shapes_resnet18_image, seed, scale_num, if_correct, bias)


def glorot_weights_resnet18_light_image(seed, scale_num=4, if_correct=True, bias=0.0):
    """glorot_weights() for ResNet18LightImage: float32 numpy arrays of Keras' shapes, [3,3,Cout,Cin] for the transposed layers."""
    return _glorot(layer_shapes_resnet18_light_image, seed, scale_num, if_correct, bias)


class _Buffers:
    """What one (device, B, H, W) needs: the weights' device copies are the instance's, these are the activations."""

    def __init__(self, device, B, H, W, scale_num, image_width=0):
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        self.new = new
        self.mask, self.scaled, self.correct = new(B, H, W), new(B, H, W), new(B, H, W)
        self.a16, self.b16, self.one = new(B, H, W, 16), new(B, H, W, 16), new(B, H, W, 1)
        self.fills = [new(B, H, W) for _ in range(scale_num - 1)]
        self.stems = new(B, H, W, image_width + STEM_WIDTH * scale_num)  # [image | stems] in the image network
        self.output, self.correct_out = new(B, H, W), new(B, H, W)


class _LidarNet:
    """What the reference's networks share: the settings, the weights dict and its checks, the device copies, and the head
    (net.py:125-212 and 464-547, the same lines twice): mask, division, correction, multi-channel fill, stems."""

    NAME = None  # the reference's class, for messages
    KNOWN = ()  # every attribute name of the reference's class
    layer_shapes = None  # (scale_num, if_correct) -> {name: (ksize, Cin, Cout)}

    def __init__(self, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4):
        self.table_size, self.if_correct, self.scale_range, self.scale_num = int(table_size), bool(if_correct), float(scale_range), scale_num
        if (self.table_size + 1) % 2 != 0:
            raise ValueError("table_size must be odd, got %r" % (table_size,))
        if not np.isfinite(self.scale_range) or self.scale_range == 0.0:
            raise ValueError("scale_range must be finite and not 0, got %r" % (scale_range,))
        self.shapes = type(self).layer_shapes(scale_num, self.if_correct)
        unknown = sorted(set(weights) - set(self.KNOWN))
        if unknown:
            raise ValueError("not a layer of %s: %s" % (self.NAME, ", ".join(unknown)))
        self._host = {}
        for name, (k, cin, cout) in self.shapes.items():
            if name not in weights:
                raise ValueError("weights lack layer %r" % name)
            kernel, bias = (np.ascontiguousarray(a, dtype=np.float32) for a in weights[name])
            if kernel.shape != _keras_shape(name, k, cin, cout) or bias.shape != (cout,):
                raise ValueError("layer %r needs a kernel %s and a bias %s, got %s and %s"
                                 % (name, _keras_shape(name, k, cin, cout), (cout,), kernel.shape, bias.shape))
            self._host[name] = (pack_transpose_kernel(kernel) if name in RESNET_TRANSPOSED else kernel, bias)
        self._on = {}  # device -> ({name: (kernel, bias)}, threshold, scale_range), as tensors there
        self._buffers = {}  # (device, B, H, W) -> the activations

    def _conv(self, on, x, name, act, out, out_offset=0):
        kernel, bias = on[name]
        return conv2d_device(x, kernel, bias, act, LEAKY_ALPHA, out, out_offset)

    def _state(self, dev):
        """({name: (kernel, bias)}, threshold, scale_range) as tensors on dev, uploaded on the first call there."""
        if dev not in self._on:
            up = lambda a: torch.from_numpy(a).to(dev)
            self._on[dev] = ({n: (up(k), up(b)) for n, (k, b) in self._host.items()},
                             torch.tensor(0.1, dtype=torch.float32, device=dev),
                             torch.tensor(self.scale_range, dtype=torch.float32, device=dev))
        return self._on[dev]

    def _head(self, on, threshold, scale, x, t, stem_offset=0):
        """x [B,H,W] -> t.correct, and the stems' [B,H,W,16 scale_num] in t.stems from channel stem_offset on."""
        B, H, W = x.shape
        torch.gt(x, threshold, out=t.mask)  # valued_mask, as float32
        torch.div(x, scale, out=t.scaled)  # (a tensor divisor: an IEEE division, not a product with 1 / scale_range)
        if self.if_correct:
            self._conv(on, t.scaled, "correct_1", "leaky", t.a16)
            self._conv(on, t.a16, "correct_2", "leaky", t.b16)
            self._conv(on, t.b16, "correct_3", "leaky", t.a16)
            self._conv(on, t.a16, "correct_4", "linear", t.one)
            torch.mul(t.one.view(B, H, W), t.mask, out=t.correct)
        else:
            torch.mul(t.scaled, t.mask, out=t.correct)
        lidars = _device.generate_multi_channel_device(t.correct, t.mask, self.table_size, self.scale_num, outs=t.fills)
        for k, name in enumerate(stem_layers(self.scale_num)):  # tf.concat: each stem writes its 16 channels
            self._conv(on, lidars[k], name, "leaky", t.stems, stem_offset + STEM_WIDTH * k)


class SparsityCNN(_LidarNet):
    """net.py's SparsityCNN for inference.  weights: {layer name: (kernel, bias)} under the reference's attribute names
    (correct_1..4 with if_correct, lidar_conv, lidar_conv_extra_1..2 as scale_num asks, conv1a..d, conv_output), kernel
    [ksize,ksize,Cin,Cout] and bias [Cout] as Keras stores them (layer.get_weights()), float32.  lidar_conv_extra_3 and layers
    the settings do not use are accepted and ignored; a name the reference's class does not have raises.

    Calling it is detached: this class is inference only, no gradient flows through it.  It synchronises nothing with the host
    and, after the first call at a shape, allocates no activation buffer: the two tensors it returns are the instance's own for
    that shape and the next call at that shape overwrites them, so clone what has to outlive it.  One instance serves one stream
    at a time."""

    NAME = "SparsityCNN"
    KNOWN = _KNOWN
    layer_shapes = staticmethod(layer_shapes)

    def __call__(self, input_lidar):
        """input_lidar: contiguous float32 CUDA tensor [B,H,W] in metres.  Returns (output * scale_range, lidar_correct *
        scale_range), net.py:242, each [B,H,W]."""
        x = input_lidar.detach()
        _check_tensor(x, "input_lidar")
        B, H, W = x.shape
        dev = x.device
        with torch.cuda.device(dev):
            on, threshold, scale = self._state(dev)
            key = (dev, B, H, W)
            if key not in self._buffers:
                self._buffers[key] = _Buffers(dev, B, H, W, self.scale_num)
            t = self._buffers[key]
            self._head(on, threshold, scale, x, t)
            self._conv(on, t.stems, "conv1a", "leaky", t.a16)
            self._conv(on, t.a16, "conv1b", "leaky", t.b16)
            self._conv(on, t.b16, "conv1c", "leaky", t.a16)
            self._conv(on, t.a16, "conv1d", "leaky", t.b16)
            self._conv(on, t.b16, "conv_output", "linear", t.one)
            torch.mul(t.one.view(B, H, W), scale, out=t.output)
            torch.mul(t.correct, scale, out=t.correct_out)
        return t.output, t.correct_out


class _ConvVariables(torch.nn.Module):
    """The two variables of a Keras Conv2D under its attribute names: kernel [ksize,ksize,Cin,Cout] and bias [Cout]."""

    def __init__(self, kernel, bias):
        super().__init__()
        self.kernel = torch.nn.Parameter(torch.from_numpy(kernel.copy()))
        self.bias = torch.nn.Parameter(torch.from_numpy(bias.copy()))


class _TrainableNet(torch.nn.Module):
    """What the trainable networks share: the settings and the weights' checks (the inference class's), the parameters
    <layer>.kernel and <layer>.bias in Keras' layouts, and the head (net.py:125-212 and 464-547) under the tape."""

    INFERENCE = None  # the inference class whose checks and layer table these are

    def __init__(self, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4, joint_train=False):
        super().__init__()
        checked = self.INFERENCE(weights, table_size, if_correct, scale_range, scale_num)  # the settings' and the weights' checks
        self.table_size, self.if_correct, self.scale_num = checked.table_size, checked.if_correct, checked.scale_num
        self.scale_range, self.joint_train = checked.scale_range, bool(joint_train)
        for name, (k, cin, cout) in checked.shapes.items():
            kernel, bias = (np.ascontiguousarray(a, dtype=np.float32) for a in weights[name])  # Keras' layouts, not the packed one
            setattr(self, name, _ConvVariables(kernel, bias))
        self.register_buffer("_threshold", torch.tensor(0.1, dtype=torch.float32), persistent=False)
        self.register_buffer("_scale", torch.tensor(self.scale_range, dtype=torch.float32), persistent=False)

    def _conv(self, x, name, act):
        from . import autograd

        layer = getattr(self, name)
        return autograd.conv2d(x, layer.kernel, layer.bias, act, LEAKY_ALPHA)

    def _head(self, x):
        """x [B,H,W] -> (lidar_correct [B,H,W], the stems' tf.concat [B,H,W,16 scale_num])."""
        from . import autograd

        B, H, W = x.shape
        mask = torch.gt(x, self._threshold).to(torch.float32)  # valued_mask
        scaled = torch.div(x, self._scale)  # (a tensor divisor: an IEEE division, as in SparsityCNN)
        if self.if_correct:
            t = self._conv(scaled, "correct_1", "leaky")
            t = self._conv(t, "correct_2", "leaky")
            t = self._conv(t, "correct_3", "leaky")
            correct = self._conv(t, "correct_4", "linear").view(B, H, W) * mask
        else:
            correct = scaled * mask
        # The fill's input is ONE consumer of lidar_correct (the second output is the other), and has two itself (the
        # window steps, and the first stem as lidar_1): every gradient sum on the tape has two terms, so no float32 sum
        # depends on the order in which the autograd engine happens to run the nodes.
        fill_in = correct.view_as(correct) if self.joint_train else correct.detach()
        lidars = autograd.generate_multi_channel(fill_in, mask, self.table_size, self.scale_num)
        stems = [self._conv(lidars[k], name, "leaky") for k, name in enumerate(stem_layers(self.scale_num))]
        return correct, (torch.cat(stems, dim=3) if len(stems) > 1 else stems[0])  # tf.concat


class SparsityCNNTrainable(_TrainableNet):
    """net.py's SparsityCNN under a tape: the network of SparsityCNN above as a torch.nn.Module, for train.py:232-254's step
    (a forward, autograd.train_loss, backward(), an optimizer's step).  weights: as SparsityCNN takes them; they become the
    module's parameters <layer>.kernel and <layer>.bias under the reference's attribute names (correct_1.kernel, ..), in Keras'
    layouts, so a state_dict maps to layer.get_weights() name by name.  lidar_conv_extra_3 and layers the settings do not use
    are accepted and ignored, as there.  The module is built on the host: move it with .to(device).

    forward(input_lidar) returns (output * scale_range, lidar_correct * scale_range) with the bits SparsityCNN returns for the
    same weights: every convolution is autograd.conv2d (dtfill_conv2d forward, dtfill_conv2d_backward_data and _weights
    backward), the multi-channel fill is autograd.generate_multi_channel, and the mask and scale steps are single torch
    operations.  joint_train = False cuts the gradient behind the fill (net.py:157-162), so the correction branch learns from
    the auxiliary loss alone; with joint_train the fill's backward carries the main loss into it.  lidar_conv_extra_1 reads
    lidar_2 and lidar_4 (net.py:176, 206): its gradient is the sum of both uses.  Every gradient bit is a function of the
    weights, the input and the shape alone.  No host synchronisation in either direction; activations are new tensors of each
    call, as a tape needs them."""

    INFERENCE = SparsityCNN

    def forward(self, input_lidar):
        """input_lidar: contiguous float32 CUDA tensor [B,H,W] in metres, a constant.  Returns two [B,H,W] tensors."""
        x = input_lidar.detach()
        _check_tensor(x, "input_lidar")
        B, H, W = x.shape
        with torch.cuda.device(x.device):
            correct, t = self._head(x)
            for name in ("conv1a", "conv1b", "conv1c", "conv1d"):
                t = self._conv(t, name, "leaky")
            output = self._conv(t, "conv_output", "linear").view(B, H, W)
            return output * self._scale, correct * self._scale


class _ResNetBuffers(_Buffers):
    """_Buffers and, per level k (1 / 2^(k-1) of the frame each way, RESNET_WIDTHS[k-1] channels), three tensors that take turns
    and the wide tensor a tf.concat([up, skip]) of that level is."""

    def __init__(self, device, B, H, W, scale_num, image_width=0):
        super().__init__(device, B, H, W, scale_num, image_width)
        self.level, self.wide = [], []
        for k, width in enumerate(RESNET_WIDTHS):
            frame = (B, H >> k, W >> k)
            self.level.append([self.new(*frame, width) for _ in range(3)])
            if k < 3:  # [up | skip]: level 1's is upsample_1's 64 channels and the stems, the others twice the level's width
                self.wide.append(self.new(*frame, 64 + image_width + STEM_WIDTH * scale_num if k == 0 else 2 * width))
        self.wide1 = self.new(B, H, W, 128)  # upsample_2's 64 channels and tensor_1_total


class ResNet18(_LidarNet):
    """net.py's ResNet18_NO_BN_l2 (net.py:245-745, the paper's network) for inference.  weights: {layer name: (kernel, bias)}
    under the reference's attribute names (layer_shapes_resnet18: correct_1..4, the stems, conv1a .. conv4d,
    conv1a_extra .. conv4a_extra, upsample_4 .. upsample_1, upsample_1_post .. upsample_4_post, conv_output), as Keras stores
    them (layer.get_weights()): [ksize,ksize,Cin,Cout], and [3,3,Cout,Cin] for the three Conv2DTranspose layers, which are
    repacked once here (pack_transpose_kernel).  lidar_conv_extra_3 is accepted and ignored, as the reference builds it and
    calls lidar_conv_extra_1 on lidar_4 instead (net.py:541); a name the reference's class does not have raises.

    The head is SparsityCNN's.  A residual block's tensor + tensor_add and the leaky_relu after it are the convolution's own
    finish (dtfill_conv2d_strided's residual).  Each tf.concat([up, skip]) is the transposed convolution (at level 1, the
    convolution upsample_1) writing the channels from 0 of a wide tensor, and one strided torch copy of the skip tensor into
    the channels above: one memory pass beside a layer of hundreds of MFLOP per kilopixel.

    H and W must be multiples of 8: with any other size the reference's own concat fails.  Detached, no host synchronisation,
    no activation buffer allocated after the first call at a shape, the returned tensors are the instance's own, one stream
    at a time: as SparsityCNN."""

    NAME = "ResNet18_NO_BN_l2"
    KNOWN = tuple(layer_shapes_resnet18(4, True)) + ("lidar_conv_extra_3",)
    layer_shapes = staticmethod(layer_shapes_resnet18)

    def _wide(self, on, x, name, out, stride=1, residual=None, act="leaky"):
        kernel, bias = on[name]
        return conv2d_strided_device(x, kernel, bias, stride, residual, act, LEAKY_ALPHA, out)

    def _up(self, on, x, name, out):
        kernel, bias = on[name]
        return conv2d_transpose_device(x, kernel, bias, "leaky", LEAKY_ALPHA, out)

    IMAGE_WIDTH = 0  # channels of an image layer in front of the stems (ResNet18Image)

    def __call__(self, input_lidar):
        """input_lidar: contiguous float32 CUDA tensor [B,H,W] in metres, H and W multiples of 8.  Returns (output *
        scale_range, lidar_correct * scale_range), net.py:745, each [B,H,W]."""
        return self._run(input_lidar, None)

    def _run(self, input_lidar, rgb):
        """The forward of both networks; rgb: the image network's second input, already detached, or None."""
        x = input_lidar.detach()
        if x.dim() == 3 and (x.shape[1] % 8 or x.shape[2] % 8):
            raise ValueError("H and W must be multiples of 8, got %d x %d" % tuple(x.shape[1:]))
        _check_tensor(x, "input_lidar")
        B, H, W = x.shape
        dev = x.device
        if rgb is not None:
            _check_tensor(rgb, "input_rgb", layout="[B,H,W,3]")
            if tuple(rgb.shape) != (B, H, W, 3) or rgb.device != dev:
                raise ValueError("input_rgb must be [%d,%d,%d,3] on %s, got %s" % (B, H, W, dev, tuple(rgb.shape)))
        with torch.cuda.device(dev):
            on, threshold, scale = self._state(dev)
            key = (dev, B, H, W)
            if key not in self._buffers:
                self._buffers[key] = _ResNetBuffers(dev, B, H, W, self.scale_num, self.IMAGE_WIDTH)
            t = self._buffers[key]
            self._head(on, threshold, scale, x, t, self.IMAGE_WIDTH)
            if rgb is not None:  # net.py:3645-3649: tf.concat([img_conv_1, lidar_conv_total]), the image's channels first
                kernel, bias = on["img_conv"]
                conv2d_image_device(rgb, kernel, bias, "leaky", LEAKY_ALPHA, t.stems, 0)
            below = t.stems
            for k in range(4):  # net.py:551-674; `below` ends as tensor_<k+1>_total (level 4: tensor_4)
                p, q, r = t.level[k]
                name, stride = "conv%d" % (k + 1), 1 if k == 0 else 2
                self._wide(on, below, name + "a", p, stride)
                self._wide(on, below, name + "a_extra", q, stride, act="linear")
                self._wide(on, p, name + "b", r, residual=q)
                self._wide(on, r, name + "c", p)
                self._wide(on, p, name + "d", q, residual=r if k < 3 else None)
                below = q
            for k in (2, 1, 0):  # net.py:680-724: upsample_<k+2>, the concat with tensor_<k+1>_total, upsample_<k+2>_post
                wide = t.wide1 if k == 0 else t.wide[k]
                width = RESNET_WIDTHS[k]
                self._up(on, below, "upsample_%d" % (k + 2), wide)
                wide[..., width:].copy_(t.level[k][1])
                below = self._wide(on, wide, "upsample_%d_post" % (k + 2), t.level[k][0])
            wide = t.wide[0]  # net.py:728-742
            self._wide(on, below, "upsample_1", wide)
            wide[..., 64:].copy_(t.stems)
            self._wide(on, wide, "upsample_1_post", t.level[0][2])
            self._conv(on, t.level[0][2], "conv_output", "linear", t.one)
            torch.mul(t.one.view(B, H, W), scale, out=t.output)
            torch.mul(t.correct, scale, out=t.correct_out)
        return t.output, t.correct_out


class ResNet18Image(ResNet18):
    """net.py's ResNet18_NO_BN_l2_image (net.py:3383-3893, demo.py:27's default) for inference: ResNet18 with the image beside
    the LiDAR.  The reference's class is ResNet18_NO_BN_l2 line for line but for img_conv = Conv2D(64, (3,3)) on input_rgb
    (dtfill_conv2d_image), whose leaky output is concatenated IN FRONT of the stems: conv1a, conv1a_extra and upsample_1_post
    read 64 channels more.  Here img_conv writes the channels 0 .. 63 of the stems tensor and stem k the channels 64 + 16 k on.
    weights: as ResNet18's with img_conv (layer_shapes_resnet18_image).

    Called as net(input_lidar, input_rgb); input_rgb: contiguous float32 CUDA tensor [B,H,W,3], what rgb_read_device emits
    (img_batch[:, 96:] / 255.0, demo.py:296, train.py:213).  Everything else as ResNet18: detached, no host synchronisation, no
    activation buffer allocated after the first call at a shape, the returned tensors are the instance's own."""

    NAME = "ResNet18_NO_BN_l2_image"
    KNOWN = tuple(layer_shapes_resnet18_image(4, True)) + ("lidar_conv_extra_3",)
    layer_shapes = staticmethod(layer_shapes_resnet18_image)
    IMAGE_WIDTH = IMAGE_WIDTH

    def __call__(self, input_lidar, input_rgb):
        """input_lidar: [B,H,W] in metres, H and W multiples of 8; input_rgb: [B,H,W,3].  Returns (output * scale_range,
        lidar_correct * scale_range), net.py:3893, each [B,H,W]."""
        return self._run(input_lidar, input_rgb.detach())


class _LightBuffers(_Buffers):
    """_Buffers and the light network's activations: three 64-channel tensors per level that take turns, and the tensors a
    tf.concat of the reference is.  total1: [image | conv1_pre]; pooled[k]: [the level's tensor | max_pool by k of conv1_pre]
    at 1 / k of the frame, k = 2, 4, 8; cat[n]: [upsample_n | its skip tensor], n = 4, 3, 2, 1."""

    def __init__(self, device, B, H, W, scale_num):
        super().__init__(device, B, H, W, scale_num)
        w = LIGHT_WIDTH
        self.level = [[self.new(B, H >> k, W >> k, w) for _ in range(3)] for k in range(4)]
        self.total1 = self.new(B, H, W, IMAGE_WIDTH + w)
        self.pooled = {k: self.new(B, H // k, W // k, 2 * w) for k in LIGHT_POOLS}
        self.cat = {4: self.new(B, H // 4, W // 4, 3 * w), 3: self.new(B, H // 2, W // 2, 3 * w), 2: self.new(B, H, W, 2 * w),
                    1: self.new(B, H, W, 2 * w)}


class ResNet18LightImage(ResNet18Image):
    """net.py's ResNet18_NO_BN_l2_light_image (net.py:3895-4426) for inference: the image-guided network at 64 channels on every
    level, the variant for full KITTI frames.  weights: {layer name: (kernel, bias)} under the reference's attribute names
    (layer_shapes_resnet18_light_image), as Keras stores them.  Beside the narrower layers it differs from ResNet18Image in
    this: conv1_pre, a linear 3x3 layer, folds the stems into lidar_conv_total, 64 channels; conv1a and conv1a_extra read
    [image | lidar_conv_total]; lidar_conv_total is max-pooled by 2, 4 and 8 and concatenated BEHIND tensor_2_total,
    tensor_3_total and tensor_4, and those 128-wide tensors feed the next level and the skip concats; level 4 has no second
    residual; the last concat is [upsample_1 | lidar_conv_total].

    Here conv1_pre writes the channels 64 .. 127 of the [image | total] tensor, and ONE dtfill_max_pool_pyramid call reads them
    there and writes the upper halves of the three levels' wide tensors, whose lower halves conv2d, conv3d and conv4d write: the
    three pools cost one pass over the full-resolution tensor.  Called as net(input_lidar, input_rgb); H and W multiples of 8;
    detached, no host synchronisation, no activation buffer allocated after the first call at a shape, the returned tensors are
    the instance's own: as ResNet18Image."""

    NAME = "ResNet18_NO_BN_l2_light_image"
    KNOWN = tuple(layer_shapes_resnet18_light_image(4, True)) + ("lidar_conv_extra_3",)
    layer_shapes = staticmethod(layer_shapes_resnet18_light_image)

    def _run(self, input_lidar, rgb):
        x = input_lidar.detach()
        if x.dim() == 3 and (x.shape[1] % 8 or x.shape[2] % 8):
            raise ValueError("H and W must be multiples of 8, got %d x %d" % tuple(x.shape[1:]))
        _check_tensor(x, "input_lidar")
        B, H, W = x.shape
        dev = x.device
        _check_tensor(rgb, "input_rgb", layout="[B,H,W,3]")
        if tuple(rgb.shape) != (B, H, W, 3) or rgb.device != dev:
            raise ValueError("input_rgb must be [%d,%d,%d,3] on %s, got %s" % (B, H, W, dev, tuple(rgb.shape)))
        w = LIGHT_WIDTH
        with torch.cuda.device(dev):
            on, threshold, scale = self._state(dev)
            key = (dev, B, H, W)
            if key not in self._buffers:
                self._buffers[key] = _LightBuffers(dev, B, H, W, self.scale_num)
            t = self._buffers[key]
            self._head(on, threshold, scale, x, t)
            kernel, bias = on["img_conv"]  # net.py:4166-4222: lidar_conv_total_1 = tf.concat([img_conv_1, lidar_conv_total])
            conv2d_image_device(rgb, kernel, bias, "leaky", LEAKY_ALPHA, t.total1, 0)
            kernel, bias = on["conv1_pre"]  # no leaky_relu follows it
            conv2d_strided_device(t.stems, kernel, bias, 1, None, "linear", LEAKY_ALPHA, t.total1, IMAGE_WIDTH)
            _device.max_pool_pyramid_device(t.total1, LIGHT_POOLS, IMAGE_WIDTH, w, [t.pooled[k] for k in LIGHT_POOLS], [w] * 3)
            below = t.total1
            for k in range(4):  # net.py:4224-4355; `below` ends as tensor_<k+1>_total (level 4: tensor_4), 128 wide from level 2 on
                p, q, r = t.level[k]
                name, stride = "conv%d" % (k + 1), 1 if k == 0 else 2
                out = q if k == 0 else t.pooled[1 << k]  # conv<k+1>d writes in front of the pooled channels
                self._wide(on, below, name + "a", p, stride)
                self._wide(on, below, name + "a_extra", q, stride, act="linear")
                self._wide(on, p, name + "b", r, residual=q)
                self._wide(on, r, name + "c", p)
                self._wide(on, p, name + "d", out, residual=r if k < 3 else None)
                below = out
            skips = {4: t.pooled[4], 3: t.pooled[2], 2: t.level[0][1], 1: t.total1[..., IMAGE_WIDTH:]}
            for n in (4, 3, 2):  # net.py:4360-4404: upsample_<n>, the concat with its skip tensor, upsample_<n>_post
                self._up(on, below, "upsample_%d" % n, t.cat[n])
                t.cat[n][..., w:].copy_(skips[n])
                below = self._wide(on, t.cat[n], "upsample_%d_post" % n, t.level[n - 2][0])
            self._wide(on, below, "upsample_1", t.cat[1])  # net.py:4408-4422
            t.cat[1][..., w:].copy_(skips[1])
            self._wide(on, t.cat[1], "upsample_1_post", t.level[0][2])
            self._conv(on, t.level[0][2], "conv_output", "linear", t.one)
            torch.mul(t.one.view(B, H, W), scale, out=t.output)
            torch.mul(t.correct, scale, out=t.correct_out)
        return t.output, t.correct_out


class ResNet18Trainable(_TrainableNet):
    """net.py's ResNet18_NO_BN_l2 under a tape: the network of ResNet18 above as a torch.nn.Module, the network train.py:113
    trains, for train.py:232-254's step.  weights: as ResNet18 takes them; they become the parameters <layer>.kernel and
    <layer>.bias under the reference's attribute names in Keras' layouts ([3,3,Cout,Cin] for the three Conv2DTranspose layers:
    the pack is a permute inside the graph, autograd.conv2d_transpose), so a state_dict maps to layer.get_weights() name by
    name.  Built on the host: move it with .to(device).

    forward(input_lidar) returns (output * scale_range, lidar_correct * scale_range) with the bits ResNet18 returns for the
    same weights.  The head is SparsityCNNTrainable's; the wide layers are autograd.conv2d_strided and
    autograd.conv2d_transpose, every tf.concat a torch.cat.  joint_train as in SparsityCNNTrainable.  H and W must be
    multiples of 8.  The reference declares kernel_regularizer=l2(0.05) on its layers, but train.py:253 differentiates
    total_loss alone and never adds depth_network.losses: the gradient reproduced here has no weight-decay term.

    Every float32 gradient sum the tape makes has exactly two terms, so the order in which the autograd engine runs the nodes
    cannot change a bit.  Four tensors have three consumers, the stems (conv1a, conv1a_extra, the concat in front of
    upsample_1_post) and tensor_k_total for k = 1..3 (conv(k+1)a, conv(k+1)a_extra, the concat of level k): the two
    convolutions read one identity view, so the tensor's gradient is (d conv_a + d conv_a_extra) + d concat.
    No host synchronisation in either direction; activations are new tensors of each call."""

    INFERENCE = ResNet18

    def _wide(self, x, name, stride=1, residual=None, act="leaky"):
        from . import autograd

        layer = getattr(self, name)
        return autograd.conv2d_strided(x, layer.kernel, layer.bias, stride, residual, act, LEAKY_ALPHA)

    def _up(self, x, name):
        from . import autograd

        layer = getattr(self, name)
        return autograd.conv2d_transpose(x, layer.kernel, layer.bias, "leaky", LEAKY_ALPHA)

    def forward(self, input_lidar):
        """input_lidar: contiguous float32 CUDA tensor [B,H,W] in metres, H and W multiples of 8, a constant.  Returns two
        [B,H,W] tensors."""
        return self._run(input_lidar, None)

    def _image(self, rgb):
        """The image layer's output, which stands in front of the stems (ResNet18ImageTrainable)."""
        raise NotImplementedError

    def _run(self, input_lidar, rgb):
        x = input_lidar.detach()
        if x.dim() == 3 and (x.shape[1] % 8 or x.shape[2] % 8):
            raise ValueError("H and W must be multiples of 8, got %d x %d" % tuple(x.shape[1:]))
        _check_tensor(x, "input_lidar")
        B, H, W = x.shape
        with torch.cuda.device(x.device):
            correct, stems = self._head(x)
            if rgb is not None:  # net.py:3645-3649
                stems = torch.cat([self._image(rgb), stems], dim=3)
            below, totals = stems, []
            for level in (1, 2, 3, 4):  # net.py:551-674
                name, stride = "conv%d" % level, 1 if level == 1 else 2
                both = below.view_as(below)  # ONE consumer of `below` for the two convolutions; the concat is the other
                t = self._wide(both, name + "a", stride)
                add = self._wide(both, name + "a_extra", stride, act="linear")
                total = self._wide(t, name + "b", residual=add)
                t = self._wide(total, name + "c")
                below = self._wide(t, name + "d", residual=total if level < 4 else None)
                totals.append(below)
            for level in (4, 3, 2):  # net.py:680-724
                up = torch.cat([self._up(below, "upsample_%d" % level), totals[level - 2]], dim=3)
                below = self._wide(up, "upsample_%d_post" % level)
            up = torch.cat([self._wide(below, "upsample_1"), stems], dim=3)  # net.py:728-742
            t = self._wide(up, "upsample_1_post")
            output = self._conv(t, "conv_output", "linear").view(B, H, W)
            return output * self._scale, correct * self._scale


class ResNet18ImageTrainable(ResNet18Trainable):
    """net.py's ResNet18_NO_BN_l2_image under a tape: ResNet18Image as a torch.nn.Module, ResNet18Trainable with img_conv
    (autograd.conv2d_image) in front of the stems.  weights: as ResNet18Image takes them; the parameters are <layer>.kernel and
    <layer>.bias, img_conv's among them.  forward(input_lidar, input_rgb) returns the bits ResNet18Image returns for the same
    weights.  input_rgb is a constant: the image is data, img_conv has no data gradient, and an input_rgb that requires a
    gradient raises ValueError.

    The tensor with three consumers at level 1 is now the [image | stems] concat, 64 + 16 scale_num wide: its gradient is
    (d conv1a + d conv1a_extra) + d concat, two-term sums as before; img_conv reads the channels 0 .. 63 of it in place and stem
    k the channels 64 + 16 k on (torch.cat's backward hands out slices, autograd's convolutions read them at an offset)."""

    INFERENCE = ResNet18Image

    def _image(self, rgb):
        from . import autograd

        return autograd.conv2d_image(rgb, self.img_conv.kernel, self.img_conv.bias, "leaky", LEAKY_ALPHA)

    def forward(self, input_lidar, input_rgb):
        """input_lidar: [B,H,W] in metres, H and W multiples of 8; input_rgb: contiguous float32 CUDA tensor [B,H,W,3]; both
        constants.  Returns two [B,H,W] tensors."""
        if input_rgb.requires_grad:
            raise ValueError("input_rgb is a constant: the image is data and img_conv has no data gradient; pass input_rgb.detach()")
        _check_tensor(input_rgb, "input_rgb", layout="[B,H,W,3]")
        if input_lidar.dim() == 3 and (tuple(input_rgb.shape) != tuple(input_lidar.shape) + (3,) or input_rgb.device != input_lidar.device):
            raise ValueError("input_rgb must be %s on %s, got %s" % (tuple(input_lidar.shape) + (3,), input_lidar.device, tuple(input_rgb.shape)))
        return self._run(input_lidar, input_rgb)


class ResNet18LightImageTrainable(ResNet18ImageTrainable):
    """net.py's ResNet18_NO_BN_l2_light_image under a tape: ResNet18LightImage as a torch.nn.Module over the same operators as
    ResNet18ImageTrainable and autograd.max_pool_pyramid.  weights: as ResNet18LightImage takes them; the parameters are
    <layer>.kernel and <layer>.bias in Keras' layouts.  forward(input_lidar, input_rgb) returns the bits ResNet18LightImage
    returns for the same weights; input_rgb is a constant.

    Every float32 gradient sum of the tape has two terms.  lidar_conv_total, conv1_pre's output, has three consumers, the image
    concat, the pools and the last concat: the first two read one identity view, and the three pools are ONE operator whose
    backward sums its levels in a fixed grouping, so the tensor's gradient is (d concat_image + d pools) + d concat_1.  The
    128-wide tensors of levels 2 and 3 have three consumers each, conv(k+1)a, conv(k+1)a_extra and the skip concat: the two
    convolutions read one view, as in ResNet18Trainable, as they do of tensor_1_total."""

    INFERENCE = ResNet18LightImage

    def _run(self, input_lidar, rgb):
        from . import autograd

        x = input_lidar.detach()
        if x.dim() == 3 and (x.shape[1] % 8 or x.shape[2] % 8):
            raise ValueError("H and W must be multiples of 8, got %d x %d" % tuple(x.shape[1:]))
        _check_tensor(x, "input_lidar")
        B, H, W = x.shape
        with torch.cuda.device(x.device):
            correct, stems = self._head(x)
            total = self._wide(stems, "conv1_pre", act="linear")  # lidar_conv_total, net.py:4220
            both = total.view_as(total)  # ONE consumer of it for the image concat and the pools; the last concat is the other
            pooled = dict(zip((2, 3, 4), autograd.max_pool_pyramid(both, LIGHT_POOLS)))  # level -> the pool behind its tensor
            below, totals = torch.cat([self._image(rgb), both], dim=3), []
            for level in (1, 2, 3, 4):  # net.py:4224-4355
                name, stride = "conv%d" % level, 1 if level == 1 else 2
                both = below.view_as(below)  # ONE consumer of `below` for the two convolutions; the skip concat is the other
                t = self._wide(both, name + "a", stride)
                add = self._wide(both, name + "a_extra", stride, act="linear")
                mid = self._wide(t, name + "b", residual=add)
                t = self._wide(mid, name + "c")
                below = self._wide(t, name + "d", residual=mid if level < 4 else None)
                if level > 1:
                    below = torch.cat([below, pooled[level]], dim=3)
                totals.append(below)
            for level in (4, 3, 2):  # net.py:4360-4404
                up = torch.cat([self._up(below, "upsample_%d" % level), totals[level - 2]], dim=3)
                below = self._wide(up, "upsample_%d_post" % level)
            up = torch.cat([self._wide(below, "upsample_1"), total], dim=3)  # net.py:4408-4422: lidar_conv_total, not the stems
            t = self._wide(up, "upsample_1_post")
            output = self._conv(t, "conv_output", "linear").view(B, H, W)
            return output * self._scale, correct * self._scale
