"""SparsityCNN (solution_DeepNet/net.py:11-242), the reference's light network, as an inference class on the device: every
convolution is dtfill_conv2d's fixed-order float32 chain (include/dtfill.h), the multi-channel fill in its middle is
dtfill_generate_multi_channel, and the three elementwise steps are single IEEE operations in torch.  So the output bits are a
function of the weights and the input alone, from run to run and from shape to shape.

The other eleven models of the reference's net.py need stride 2 and Conv2DTranspose and are not here.  conv2d_device, the
device function of one convolution, is reached as device.conv2d_device as well; it lives here, beside device.py's helpers, with
its argument checks in tests/test_conv2d.py and tests/test_gpu_conv2d.py.
"""
import numpy as np
import torch

from . import _lib
from . import device as _device
from .device import _check_tensor, _ptr, _require_gpu, _stream

LEAKY_ALPHA = 0.2  # tf.nn.leaky_relu's default
STEM_WIDTH = 16  # channels every stem writes of the [B,H,W,16 * scale_num] tensor conv1a reads


def conv2d_device(x, w, bias=None, act="linear", alpha=0.2, out=None, out_offset=0):
    """A stride-1 'same' float32 convolution in the fixed summation order of include/dtfill.h, dtfill_conv2d (a layer of
    net.py's SparsityCNN).  x: contiguous float32 CUDA tensor [B,H,W,Cin], or [B,H,W] for Cin = 1; w: [ksize,ksize,Cin,Cout], a
    Keras Conv2D.kernel as stored (cross-correlation); bias: [Cout] or None; act: "linear" or "leaky" (y > 0 ? y : y * alpha).
    out: a contiguous float32 tensor [B,H,W,C] on x's device of which the channels out_offset .. out_offset + Cout - 1 are
    written and the others left as they are (not x itself); a new [B,H,W,Cout] tensor by default.  Returns out.  Asynchronous on
    the current stream; the shapes the library takes are the header's (DtfillError otherwise)."""
    if act not in _lib.CONV_ACTS:
        raise ValueError("act must be one of %s, got %r" % (sorted(_lib.CONV_ACTS), act))
    _require_gpu()
    if x.dim() == 3:
        _check_tensor(x, "x")
    else:
        _check_tensor(x, "x", layout="[B,H,W,Cin]")
    B, H, W = x.shape[:3]
    Cin = x.shape[3] if x.dim() == 4 else 1
    _check_tensor(w, "w", layout="[ksize,ksize,Cin,Cout]")
    ksize, Cout = w.shape[0], w.shape[3]
    if w.shape[1] != ksize or w.shape[2] != Cin or w.device != x.device:
        raise ValueError("w must be [ksize,ksize,%d,Cout] on %s, got %s" % (Cin, x.device, tuple(w.shape)))
    if bias is not None:
        _check_tensor(bias, "bias", layout="[Cout]")
        if bias.shape[0] != Cout or bias.device != x.device:
            raise ValueError("bias must be [%d] on %s, got %s" % (Cout, x.device, tuple(bias.shape)))
    if out is None:
        if out_offset != 0:
            raise ValueError("out_offset needs an out tensor to point into")
        out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
    else:
        _check_tensor(out, "out", layout="[B,H,W,C]")
        if tuple(out.shape[:3]) != (B, H, W) or out.device != x.device:
            raise ValueError("out must be [%d,%d,%d,C] on %s, got %s" % (B, H, W, x.device, tuple(out.shape)))
        if out.data_ptr() == x.data_ptr():
            raise ValueError("out may not alias x")
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dtfill_conv2d(x.data_ptr(), B, H, W, Cin, w.data_ptr(), _ptr(bias), ksize, Cout,
                                             _lib.CONV_ACTS[act], float(alpha), out.data_ptr(), out.shape[3], int(out_offset),
                                             _stream(x.device)))
    return out


def stem_layers(scale_num):
    """The layer that reads lidar_1 .. lidar_<scale_num>, in that order.  net.py:206 calls lidar_conv_extra_1 again on
    lidar_4: lidar_conv_extra_3 is built (net.py:46) and never used, and that is reproduced here."""
    if scale_num not in (1, 2, 3, 4):
        raise ValueError("scale_num must be 1, 2, 3 or 4, got %r" % (scale_num,))
    return ("lidar_conv", "lidar_conv_extra_1", "lidar_conv_extra_2", "lidar_conv_extra_1")[:scale_num]


def layer_shapes(scale_num=4, if_correct=True):
    """{layer name: (ksize, Cin, Cout)} of the layers the forward uses, under the reference's attribute names."""
    shapes = {}
    if if_correct:
        shapes.update(correct_1=(7, 1, 16), correct_2=(5, 16, 16), correct_3=(3, 16, 16), correct_4=(3, 16, 1))
    for name in stem_layers(scale_num):
        shapes[name] = (3, 1, STEM_WIDTH)
    shapes.update(conv1a=(7, STEM_WIDTH * scale_num, 16), conv1b=(5, 16, 16), conv1c=(3, 16, 16), conv1d=(3, 16, 16),
                  conv_output=(1, 16, 1))
    return shapes


_KNOWN = tuple(layer_shapes(4, True)) + ("lidar_conv_extra_3",)  # every attribute name of the reference's class


def glorot_weights(seed, scale_num=4, if_correct=True, bias=0.0):
    """A weights dict for tests and benchmarks: Keras' default glorot_uniform kernels, uniform(+-sqrt(6 / (fan_in + fan_out))),
    and biases uniform in +-bias (Keras starts them at zero), as float32 numpy arrays of Keras' shapes.  Holds
    lidar_conv_extra_3 when the reference would build it (scale_num 4)."""
    rng = np.random.default_rng(seed)
    shapes = layer_shapes(scale_num, if_correct)
    if scale_num > 3:
        shapes["lidar_conv_extra_3"] = (3, 1, STEM_WIDTH)
    weights = {}
    for name, (k, cin, cout) in shapes.items():
        limit = np.sqrt(6.0 / (k * k * (cin + cout)))
        weights[name] = (rng.uniform(-limit, limit, (k, k, cin, cout)).astype(np.float32),
                         rng.uniform(-bias, bias, (cout,)).astype(np.float32))
    return weights


class _Buffers:
    """What one (device, B, H, W) needs: the weights' device copies are the instance's, these are the activations."""

    def __init__(self, device, B, H, W, scale_num):
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        self.mask, self.scaled, self.correct = new(B, H, W), new(B, H, W), new(B, H, W)
        self.a16, self.b16, self.one = new(B, H, W, 16), new(B, H, W, 16), new(B, H, W, 1)
        self.fills = [new(B, H, W) for _ in range(scale_num - 1)]
        self.stems = new(B, H, W, STEM_WIDTH * scale_num)
        self.output, self.correct_out = new(B, H, W), new(B, H, W)


class SparsityCNN:
    """net.py's SparsityCNN for inference.  weights: {layer name: (kernel, bias)} under the reference's attribute names
    (correct_1..4 with if_correct, lidar_conv, lidar_conv_extra_1..2 as scale_num asks, conv1a..d, conv_output), kernel
    [ksize,ksize,Cin,Cout] and bias [Cout] as Keras stores them (layer.get_weights()), float32.  lidar_conv_extra_3 and layers
    the settings do not use are accepted and ignored; a name the reference's class does not have raises.

    Calling it is detached: this class is inference only, no gradient flows through it.  It synchronises nothing with the host
    and, after the first call at a shape, allocates no activation buffer: the two tensors it returns are the instance's own for
    that shape and the next call at that shape overwrites them, so clone what has to outlive it.  One instance serves one stream
    at a time."""

    def __init__(self, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4):
        self.table_size, self.if_correct, self.scale_range, self.scale_num = int(table_size), bool(if_correct), float(scale_range), scale_num
        if (self.table_size + 1) % 2 != 0:
            raise ValueError("table_size must be odd, got %r" % (table_size,))
        if not np.isfinite(self.scale_range) or self.scale_range == 0.0:
            raise ValueError("scale_range must be finite and not 0, got %r" % (scale_range,))
        self.shapes = layer_shapes(scale_num, self.if_correct)
        unknown = sorted(set(weights) - set(_KNOWN))
        if unknown:
            raise ValueError("not a layer of SparsityCNN: %s" % ", ".join(unknown))
        self._host = {}
        for name, (k, cin, cout) in self.shapes.items():
            if name not in weights:
                raise ValueError("weights lack layer %r" % name)
            kernel, bias = (np.ascontiguousarray(a, dtype=np.float32) for a in weights[name])
            if kernel.shape != (k, k, cin, cout) or bias.shape != (cout,):
                raise ValueError("layer %r needs a kernel %s and a bias %s, got %s and %s"
                                 % (name, (k, k, cin, cout), (cout,), kernel.shape, bias.shape))
            self._host[name] = (kernel, bias)
        self._on = {}  # device -> ({name: (kernel, bias)}, threshold, scale_range), as tensors there
        self._buffers = {}  # (device, B, H, W) -> _Buffers

    def _conv(self, on, x, name, act, out, out_offset=0):
        kernel, bias = on[name]
        return conv2d_device(x, kernel, bias, act, LEAKY_ALPHA, out, out_offset)

    def __call__(self, input_lidar):
        """input_lidar: contiguous float32 CUDA tensor [B,H,W] in metres.  Returns (output * scale_range, lidar_correct *
        scale_range), net.py:242, each [B,H,W]."""
        x = input_lidar.detach()
        _check_tensor(x, "input_lidar")
        B, H, W = x.shape
        dev = x.device
        with torch.cuda.device(dev):
            if dev not in self._on:
                up = lambda a: torch.from_numpy(a).to(dev)
                self._on[dev] = ({n: (up(k), up(b)) for n, (k, b) in self._host.items()},
                                 torch.tensor(0.1, dtype=torch.float32, device=dev),
                                 torch.tensor(self.scale_range, dtype=torch.float32, device=dev))
            on, threshold, scale = self._on[dev]
            key = (dev, B, H, W)
            if key not in self._buffers:
                self._buffers[key] = _Buffers(dev, B, H, W, self.scale_num)
            t = self._buffers[key]
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
                self._conv(on, lidars[k], name, "leaky", t.stems, STEM_WIDTH * k)
            self._conv(on, t.stems, "conv1a", "leaky", t.a16)
            self._conv(on, t.a16, "conv1b", "leaky", t.b16)
            self._conv(on, t.b16, "conv1c", "leaky", t.a16)
            self._conv(on, t.a16, "conv1d", "leaky", t.b16)
            self._conv(on, t.b16, "conv_output", "linear", t.one)
            torch.mul(t.one.view(B, H, W), scale, out=t.output)
            torch.mul(t.correct, scale, out=t.correct_out)
        return t.output, t.correct_out
