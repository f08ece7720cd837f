"""The max-pool pyramid on the device: tf.nn.max_pool of one tensor by 2, 4 and 8 in one pass, and its gradient (include/dtfill.h,
dtfill_max_pool_pyramid and dtfill_max_pool_pyramid_backward; csrc/dtfill_pool.hpp), what net.py's ResNet18_NO_BN_l2_light_image does
with conv1_pre's output (solution_DeepNet/net.py:4285, 4320, 4353).  The two functions are reached as device.<name> as well; they
live here, beside device.py's helpers, as the point projection's and the convolutions' do in their modules.
"""
import torch

from . import _lib
from .device import _check_tensor, _ptr, _require_gpu, _stream


def _pool_args(x, levels, x_offset, channels, tensors, offsets, what):
    """The checks the two pool functions share.  Returns (B, H, W, C, per level of _lib.POOL_LEVELS: (tensor or None, width,
    offset)); tensors and offsets run along `levels`."""
    _require_gpu()
    _check_tensor(x, "x", layout="[B,H,W,C]")
    levels = tuple(levels)
    if not levels or len(set(levels)) != len(levels) or any(k not in _lib.POOL_LEVELS for k in levels):
        raise ValueError("levels must be distinct values of %s, got %r" % (_lib.POOL_LEVELS, levels))
    tensors = [None] * len(levels) if tensors is None else list(tensors)
    offsets = [0] * len(levels) if offsets is None else [int(o) for o in offsets]
    if len(tensors) != len(levels) or len(offsets) != len(levels):
        raise ValueError("%s and their offsets must run along levels %r" % (what, levels))
    B, H, W, Cx = x.shape
    C = Cx - int(x_offset) if channels is None else int(channels)
    slots = {k: (None, 0, 0) for k in _lib.POOL_LEVELS}
    for k, t, o in zip(levels, tensors, offsets):
        if t is None:
            if o != 0:
                raise ValueError("an offset needs a tensor to point into (level %d)" % k)
            continue
        _check_tensor(t, "%s[level %d]" % (what, k), layout="[B,H/k,W/k,C]")
        if tuple(t.shape[:3]) != (B, H // k, W // k) or H % k or W % k or t.device != x.device:
            raise ValueError("%s[level %d] must be [%d,H/%d,W/%d,C] of a frame %d x %d on %s, got %s"
                             % (what, k, B, k, k, H, W, x.device, tuple(t.shape)))
        if t.data_ptr() == x.data_ptr():
            raise ValueError("%s[level %d] may not alias x" % (what, k))
        slots[k] = (t, t.shape[3], o)
    return B, H, W, C, levels, tensors, [slots[k] for k in _lib.POOL_LEVELS]


def max_pool_pyramid_device(x, levels=(2, 4, 8), x_offset=0, channels=None, outs=None, out_offsets=None):
    """tf.nn.max_pool(x, k, k, 'SAME') for every k of `levels` in ONE pass over x (include/dtfill.h, dtfill_max_pool_pyramid): what
    net.py's ResNet18_NO_BN_l2_light_image does with conv1_pre's output.  x: contiguous float32 CUDA tensor [B,H,W,Cx], of which
    the channels x_offset .. x_offset + channels - 1 are pooled (default: all from x_offset on); levels: distinct values of
    (2, 4, 8); H and W multiples of the largest.  outs: per level a contiguous float32 tensor [B,H/k,W/k,C'] whose channels
    out_offsets[i] .. + channels - 1 are written and the others left as they are (tf.concat), or None for a new [B,H/k,W/k,
    channels] tensor.  The winner of a window is the first NaN if it holds one, else the raster-first maximum; the output is
    its bits.  Returns the outs as a tuple along `levels`.  Asynchronous on the current stream; the shapes the library takes are
    the header's (DtfillError otherwise)."""
    B, H, W, C, levels, outs, slots = _pool_args(x, levels, x_offset, channels, outs, out_offsets, "outs")
    for n, k in enumerate(levels):  # (a frame that is no multiple of k is the library's to refuse)
        if outs[n] is None:
            outs[n] = torch.empty((B, H // k, W // k, max(C, 0)), dtype=torch.float32, device=x.device)
            slots[_lib.POOL_LEVELS.index(k)] = (outs[n], max(C, 0), 0)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dtfill_max_pool_pyramid(x.data_ptr(), B, H, W, C, x.shape[3], int(x_offset),
                                                       *(v for t, width, at in slots for v in (_ptr(t), width, at)), _stream(x.device)))
    return tuple(outs)


def max_pool_pyramid_backward_device(x, grads, levels=(2, 4, 8), x_offset=0, channels=None, grad_offsets=None):
    """The gradient of max_pool_pyramid_device with respect to the pooled channels of x (include/dtfill.h,
    dtfill_max_pool_pyramid_backward).  x: the forward's input, read at x_offset likewise; grads: per level of `levels` the
    gradient of that level's output, a contiguous float32 tensor [B,H/k,W/k,C'] read at grad_offsets[i] .. + channels - 1, or
    None (+0).  The winners are found again from x; dx[p] = (t_2 + t_4) + t_8 in float32, t_k the level's gradient where p is
    its window's winner and +0 elsewhere, so every bit is a function of the inputs alone.  Returns dx, a new dense [B,H,W,
    channels] tensor, every element written.  Asynchronous on the current stream, no workspace."""
    B, H, W, C, levels, grads, slots = _pool_args(x, levels, x_offset, channels, grads, grad_offsets, "grads")
    dx = torch.empty((B, H, W, max(C, 0)), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dtfill_max_pool_pyramid_backward(x.data_ptr(), B, H, W, C, x.shape[3], int(x_offset),
                                                                *(v for t, width, at in slots for v in (_ptr(t), width, at)),
                                                                dx.data_ptr(), _stream(x.device)))
    return dx
