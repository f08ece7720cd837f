"""The reference's networks (solution_DeepNet/net.py) on the device, each twice: an inference class that writes into its own
buffers, and the same network under a tape, a torch.nn.Module, for train.py:232-254's step.  Every convolution is a fixed-order
float32 chain of include/dtfill.h through conv.py's device functions (inference) or autograd.py's operators over the same
kernels (tape); the multi-channel fill in the middle is dtfill_generate_multi_channel, and the elementwise steps are single
IEEE operations in torch.  So the output and gradient bits are a function of the weights and the input alone, from run to run
and from shape to shape, and the two worlds return the same output bits.

The head (mask, division, correction branch, multi-channel fill, stems) is the same lines in every class of the reference: it
is _LidarNet._head for inference and _TrainableNet._head under the tape.  Behind it:

  SparsityCNN, SparsityCNNTrainable          net.py:11-242: five narrow layers.
  ResNet18, ResNet18Trainable                ResNet18_NO_BN_l2, net.py:245-745, the paper's network.
  ResNet18Image, ..ImageTrainable            ResNet18_NO_BN_l2_image, net.py:3383-3893, demo.py's default: img_conv reads the RGB.
  ResNet18LightImage, ..LightImageTrainable  ResNet18_NO_BN_l2_light_image, net.py:3895-4426: 64 channels on every level, and
                                             conv1_pre's output pooled by 2, 4 and 8 (ONE dtfill_max_pool_pyramid call).

The three ResNets are ONE trunk: four encoder levels (conv<k>a, a_extra, b, c, d with the residual rule), three upsample_n /
concat / upsample_n_post steps, upsample_1 and conv_output.  They differ in a few class-level FACTS, stated on the inference
class (IMAGE_WIDTH, WIDTHS, PRE, POOLS, LIDAR_SKIP; _ResNet explains them) and read from there by everything else: the layer
table (_ResNet.layer_shapes), the activation buffers (_ResNetBuffers), the inference trunk (_ResNet._run) and the tape trunk
(_ResNetTrainable._run).  ResNet18_NO_BN_l2_large_image, whose layers are all here (no pooling, no stride-4 or stride-8
layer), would be another set of facts.  The other seven models of the reference's net.py are not here.

The layer code lives in conv.py; its names are importable from here as before.
"""
import numpy as np
import torch

from . import device as _device
from .conv import (_Kind, _KINDS, _backward_data, _backward_weights, _check_act, _check_backward_kind,  # noqa: F401 (re-exported)
                   _check_conv_args, _check_conv_backward, _check_conv_out, _check_conv_slice, _convb_ws, _forward, _uploaded,
                   conv2d_backward_data_device, conv2d_backward_weights_device, conv2d_backward_workspace_bytes, conv2d_device,
                   conv2d_image, conv2d_image_backward_weights_device, conv2d_image_backward_workspace_bytes, conv2d_image_device,
                   conv2d_strided, conv2d_strided_backward_data_device, conv2d_strided_backward_weights_device,
                   conv2d_strided_bf16, conv2d_strided_bf16_device, conv2d_strided_device, conv2d_transpose,
                   conv2d_transpose_backward_data_device, conv2d_transpose_backward_weights_device, conv2d_transpose_bf16,
                   conv2d_transpose_bf16_device, conv2d_transpose_device, conv2d_wide_backward_workspace_bytes, pack_bf16_device,
                   pack_transpose_kernel, conv2d_strided_backward_data_bf16, conv2d_strided_backward_data_bf16_device,
                   conv2d_strided_backward_weights_bf16, conv2d_strided_backward_weights_bf16_device,
                   conv2d_transpose_backward_data_bf16, conv2d_transpose_backward_data_bf16_device,
                   conv2d_transpose_backward_weights_bf16, conv2d_transpose_backward_weights_bf16_device,
                   conv2d_wide_backward_bf16_workspace_bytes)
from .device import _check_tensor

LEAKY_ALPHA = 0.2  # tf.nn.leaky_relu's default
STEM_WIDTH = 16  # channels every stem writes of the [B,H,W,16 * scale_num] tensor conv1a reads
RESNET_WIDTHS = (64, 128, 256, 512)  # channels of levels 1 .. 4; level k lives at 1 / 2^(k-1) of the frame each way
RESNET_STRIDE2 = ("conv2a", "conv2a_extra", "conv3a", "conv3a_extra", "conv4a", "conv4a_extra")
RESNET_TRANSPOSED = ("upsample_4", "upsample_3", "upsample_2")  # Conv2DTranspose: Keras stores [3,3,Cout,Cin]
PRECISIONS = ("float32", "bf16")  # of the ResNets' wide and transposed layers (conv.PRECISIONS); everything else is float32 in both
IMAGE_WIDTH = 64  # channels img_conv writes in front of the stems: conv1a of the image network reads [image | stems]
LIGHT_WIDTH = 64  # channels of every level of the light network, and of conv1_pre's output, the tensor it pools
LIGHT_POOLS = (2, 4, 8)  # tf.nn.max_pool of conv1_pre's output behind levels 2, 3 and 4 (net.py:4285, 4320, 4353)


def stem_layers(scale_num):
    """The layer that reads lidar_1 .. lidar_<scale_num>, in that order.  net.py:206 calls lidar_conv_extra_1 again on
    lidar_4: lidar_conv_extra_3 is built (net.py:46) and never used, and that is reproduced here."""
    if scale_num not in (1, 2, 3, 4):
        raise ValueError("scale_num must be 1, 2, 3 or 4, got %r" % (scale_num,))
    return ("lidar_conv", "lidar_conv_extra_1", "lidar_conv_extra_2", "lidar_conv_extra_1")[:scale_num]


def _head_shapes(scale_num, if_correct):
    """The layers of the head the networks share: the correction branch and the stems."""
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


def _keras_shape(name, k, cin, cout):
    return (k, k, cout, cin) if name in RESNET_TRANSPOSED else (k, k, cin, cout)


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


def _checked_lidar(input_lidar):
    """input_lidar of a ResNet, detached: [B,H,W] with H and W multiples of 8 (with any other size the reference's own concat
    fails), refused before any device work."""
    x = input_lidar.detach()
    if x.dim() == 3 and (x.shape[1] % 8 or x.shape[2] % 8):
        raise ValueError("H and W must be multiples of 8, got %d x %d" % tuple(x.shape[1:]))
    _check_tensor(x, "input_lidar")
    return x


def _check_rgb(rgb, x):
    """input_rgb beside a checked input_lidar x: [B,H,W,3] on its device."""
    _check_tensor(rgb, "input_rgb", layout="[B,H,W,3]")
    if tuple(rgb.shape) != tuple(x.shape) + (3,) or rgb.device != x.device:
        raise ValueError("input_rgb must be [%d,%d,%d,3] on %s, got %s" % (*x.shape, x.device, tuple(rgb.shape)))


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
    KNOWN = ()  # every attribute name of the reference's class: the layers of its largest settings and the stem it never calls
    layer_shapes = None  # (scale_num, if_correct) -> {name: (ksize, Cin, Cout)}

    def __init_subclass__(cls):
        cls.KNOWN = tuple(cls.layer_shapes(4, True)) + ("lidar_conv_extra_3",)

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

    INFERENCE = None  # the inference class whose checks, layer table and facts these are

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
    """_Buffers and a ResNet's activations, sized from the layer table.  level[k]: three tensors of level k + 1's width that
    take turns, at 1 / 2^k of the frame each way.  total1: [image | lidar part], the tensor conv1a reads: `stems` itself, unless
    a PRE layer folds the stems; then the stems keep a tensor of their own and total1 is [image | the PRE layer's output].
    pooled[f]: [level tensor | max_pool by f of the lidar part] at 1 / f of the frame, for each f of POOLS.  cat[n]: [upsample_n
    | its skip tensor], n = 4, 3, 2, 1, as wide as upsample_<n>_post reads."""

    def __init__(self, device, B, H, W, net):
        image, shapes = net.IMAGE_WIDTH, net.shapes
        super().__init__(device, B, H, W, net.scale_num, 0 if net.PRE else image)
        widths = [shapes["conv%db" % level][2] for level in (1, 2, 3, 4)]
        self.level = [[self.new(B, H >> k, W >> k, widths[k]) for _ in range(3)] for k in range(4)]
        self.total1 = self.new(B, H, W, image + shapes[net.PRE][2]) if net.PRE else self.stems
        lidar = self.total1.shape[3] - image
        self.pooled = {f: self.new(B, H // f, W // f, widths[f.bit_length() - 1] + lidar) for f in net.POOLS}
        self.cat = {n: self.new(B, H >> max(n - 2, 0), W >> max(n - 2, 0), shapes["upsample_%d_post" % n][1]) for n in (4, 3, 2, 1)}


class _ResNet(_LidarNet):
    """The trunk of the reference's ResNets for inference, and the facts that tell them apart (the defaults are
    ResNet18_NO_BN_l2's).  The base tensor, which conv1a and conv1a_extra read, is [image | lidar part].

    IMAGE_WIDTH  channels img_conv (dtfill_conv2d_image, on the second input) writes in front of the lidar part; 0: no image.
    WIDTHS       channels of levels 1 .. 4.
    PRE          the linear 3x3 layer that folds the stems into the lidar part, WIDTHS[0] channels; None: the stems ARE the
                 lidar part, written there directly.
    POOLS        factors f = 2^k by which the lidar part is max-pooled and concatenated BEHIND level k + 1's tensor, which then
                 feeds the next level and the skip concat that wide; all by ONE dtfill_max_pool_pyramid call.
    LIDAR_SKIP   the last concat is [upsample_1 | lidar part]; False: [upsample_1 | the whole base tensor].

    A residual block's tensor + tensor_add and the leaky_relu after it are the convolution's own finish (dtfill_conv2d_strided's
    residual); level 4 has no second residual.  Each tf.concat([up, skip]) is the transposed convolution (at level 1, the
    convolution upsample_1) writing the channels from 0 of a cat tensor, and one strided torch copy of the skip tensor into the
    channels above: one memory pass beside a layer of hundreds of MFLOP per kilopixel.  A concat in FRONT of a layer's input
    costs nothing: img_conv writes the channels 0 .. IMAGE_WIDTH - 1 of the base tensor and the stems (or PRE) the channels
    behind; conv<k>d of a pooled level writes the channels from 0 of pooled[f], whose upper channels the pyramid call wrote.

    precision: "float32", the default, is the fixed-order float32 chain in every layer.  "bf16" runs the layers that go through
    _wide and _up (every layer of the trunk but img_conv and conv_output) on the bf16 matrix cores with float32 accumulation
    (dtfill_conv2d_strided_bf16, dtfill_conv2d_transpose_bf16) over weights packed once per device; the activations stay
    float32 in memory, so the buffers, the concat offsets and the skip copies are the same, and the head, the fill, the stems,
    the correction branch, img_conv, the pooling and conv_output stay float32.  The Trainable classes have no such argument:
    they have a settable attribute, model.precision = "bf16" (ResNet18Trainable), and pack the kernels inside every call,
    because they change every step."""

    IMAGE_WIDTH, WIDTHS, PRE, POOLS, LIDAR_SKIP = 0, RESNET_WIDTHS, None, (), False

    def __init__(self, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4, precision="float32"):
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s, got %r" % (PRECISIONS, precision))
        super().__init__(weights, table_size, if_correct, scale_range, scale_num)
        self.precision = precision
        head = set(_head_shapes(scale_num, self.if_correct)) | {"img_conv", "conv_output"}
        self.wide_layers = tuple(n for n in self.shapes if n not in head)  # the layers _wide and _up run
        self._packed = {}  # device -> {name: the packed bf16 kernel}, under "bf16"

    def _state(self, dev):
        """_LidarNet._state; under "bf16" the wide layers' kernels are packed on dev behind their upload, once."""
        state = super()._state(dev)
        if self.precision == "bf16" and dev not in self._packed:
            with torch.cuda.device(dev):
                self._packed[dev] = {n: pack_bf16_device(state[0][n][0], n in RESNET_TRANSPOSED) for n in self.wide_layers}
        return state

    @classmethod
    def layer_shapes(cls, scale_num=4, if_correct=True):
        """{layer name: (ksize, Cin, Cout)} of the layers the forward uses, under the reference's attribute names.  The key
        order is the order of the module's parameters and of glorot_weights_*'s draws: img_conv stands with PRE in front of the
        levels where there is one, and last where there is none."""
        shapes = _head_shapes(scale_num, if_correct)
        image = {"img_conv": (3, 3, cls.IMAGE_WIDTH)} if cls.IMAGE_WIDTH else {}
        lidar = STEM_WIDTH * scale_num
        if cls.PRE:
            shapes.update(image)
            shapes[cls.PRE] = (3, lidar, cls.WIDTHS[0])
            lidar = cls.WIDTHS[0]
        below, totals = cls.IMAGE_WIDTH + lidar, []  # totals: what each level hands on, the pooled channels included
        for level, width in enumerate(cls.WIDTHS, 1):
            shapes["conv%da" % level] = (3, below, width)
            shapes["conv%db" % level] = (3, width, width)
            shapes["conv%da_extra" % level] = (1, below, width)
            shapes["conv%dc" % level] = (3, width, width)
            shapes["conv%dd" % level] = (3, width, width)
            below = width + (lidar if 1 << (level - 1) in cls.POOLS else 0)
            totals.append(below)
        for n in (4, 3, 2):
            shapes["upsample_%d" % n] = (3, below, cls.WIDTHS[n - 2])
            shapes["upsample_%d_post" % n] = (3, cls.WIDTHS[n - 2] + totals[n - 2], cls.WIDTHS[n - 2])
            below = cls.WIDTHS[n - 2]
        shapes["upsample_1"] = (3, below, below)
        shapes["upsample_1_post"] = (3, below + lidar + (0 if cls.LIDAR_SKIP else cls.IMAGE_WIDTH), below)
        shapes["conv_output"] = (1, below, 1)
        if not cls.PRE:
            shapes.update(image)
        return shapes

    def _wide(self, on, x, name, out, stride=1, residual=None, act="leaky", out_offset=0):
        kernel, bias = on[name]
        if self.precision == "bf16":
            return conv2d_strided_bf16_device(x, self._packed[x.device][name], bias, stride, residual, act, LEAKY_ALPHA, out, out_offset)
        return conv2d_strided_device(x, kernel, bias, stride, residual, act, LEAKY_ALPHA, out, out_offset)

    def _up(self, on, x, name, out):
        kernel, bias = on[name]
        if self.precision == "bf16":
            return conv2d_transpose_bf16_device(x, self._packed[x.device][name], bias, "leaky", LEAKY_ALPHA, out)
        return conv2d_transpose_device(x, kernel, bias, "leaky", LEAKY_ALPHA, out)

    def _run(self, input_lidar, rgb):
        """The forward of every ResNet; rgb: the image networks' second input, already detached (unread without an image)."""
        x = _checked_lidar(input_lidar)
        B, H, W = x.shape
        dev, image = x.device, self.IMAGE_WIDTH
        if image:
            _check_rgb(rgb, x)
        with torch.cuda.device(dev):
            on, threshold, scale = self._state(dev)
            key = (dev, B, H, W)
            if key not in self._buffers:
                self._buffers[key] = _ResNetBuffers(dev, B, H, W, self)
            t = self._buffers[key]
            self._head(on, threshold, scale, x, t, 0 if self.PRE else image)
            if image:  # net.py:3645-3649, 4222: tf.concat([img_conv_1, lidar_conv_total]), the image's channels first
                kernel, bias = on["img_conv"]
                conv2d_image_device(rgb, kernel, bias, "leaky", LEAKY_ALPHA, t.total1, 0)
            if self.PRE:  # net.py:4220; no leaky_relu follows it
                self._wide(on, t.stems, self.PRE, t.total1, act="linear", out_offset=image)
            if self.POOLS:
                lidar = t.total1.shape[3] - image
                _device.max_pool_pyramid_device(t.total1, self.POOLS, image, lidar, [t.pooled[f] for f in self.POOLS],
                                                [t.pooled[f].shape[3] - lidar for f in self.POOLS])
            below, totals = t.total1, []
            for k in range(4):  # net.py:551-674, 4224-4355; `below` ends as tensor_<k+1>_total (level 4: tensor_4)
                p, q, r = t.level[k]
                name, stride = "conv%d" % (k + 1), 1 if k == 0 else 2
                out = t.pooled.get(1 << k, q)  # conv<k+1>d of a pooled level writes in front of the pooled channels
                self._wide(on, below, name + "a", p, stride)
                self._wide(on, below, name + "a_extra", q, stride, act="linear")
                self._wide(on, p, name + "b", r, residual=q)
                self._wide(on, r, name + "c", p)
                self._wide(on, p, name + "d", out, residual=r if k < 3 else None)
                below = out
                totals.append(out)
            for n in (4, 3, 2):  # net.py:680-724, 4360-4404: upsample_<n>, the concat with level n - 1's tensor, upsample_<n>_post
                cat = t.cat[n]
                self._up(on, below, "upsample_%d" % n, cat)
                cat[..., self.shapes["upsample_%d" % n][2]:].copy_(totals[n - 2])
                below = self._wide(on, cat, "upsample_%d_post" % n, t.level[n - 2][0])
            cat = t.cat[1]  # net.py:728-742, 4408-4422
            self._wide(on, below, "upsample_1", cat)
            cat[..., self.shapes["upsample_1"][2]:].copy_(t.total1[..., image:] if self.LIDAR_SKIP else t.total1)
            self._wide(on, cat, "upsample_1_post", t.level[0][2])
            self._conv(on, t.level[0][2], "conv_output", "linear", t.one)
            torch.mul(t.one.view(B, H, W), scale, out=t.output)
            torch.mul(t.correct, scale, out=t.correct_out)
        return t.output, t.correct_out


class ResNet18(_ResNet):
    """net.py's ResNet18_NO_BN_l2 (net.py:245-745, the paper's network) for inference.  weights: {layer name: (kernel, bias)}
    under the reference's attribute names (layer_shapes_resnet18: correct_1..4, the stems, conv1a .. conv4d,
    conv1a_extra .. conv4a_extra, upsample_4 .. upsample_1, upsample_1_post .. upsample_4_post, conv_output), as Keras stores
    them (layer.get_weights()): [ksize,ksize,Cin,Cout], and [3,3,Cout,Cin] for the three Conv2DTranspose layers, which are
    repacked once here (pack_transpose_kernel).  lidar_conv_extra_3 is accepted and ignored, as the reference builds it and
    calls lidar_conv_extra_1 on lidar_4 instead (net.py:541); a name the reference's class does not have raises.

    The head is SparsityCNN's, the trunk _ResNet's.  H and W must be multiples of 8: with any other size the reference's own
    concat fails.  Detached, no host synchronisation, no activation buffer allocated after the first call at a shape, the
    returned tensors are the instance's own, one stream at a time: as SparsityCNN.  precision = "bf16" (default "float32") runs
    the trunk's wide and transposed layers on the bf16 matrix cores (_ResNet has what that changes and what it does not); the
    image networks below take it too."""

    NAME = "ResNet18_NO_BN_l2"

    def __call__(self, input_lidar):
        """input_lidar: contiguous float32 CUDA tensor [B,H,W] in metres, H and W multiples of 8.  Returns (output *
        scale_range, lidar_correct * scale_range), net.py:745, each [B,H,W]."""
        return self._run(input_lidar, None)


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
    IMAGE_WIDTH = IMAGE_WIDTH

    def __call__(self, input_lidar, input_rgb):
        """input_lidar: [B,H,W] in metres, H and W multiples of 8; input_rgb: [B,H,W,3].  Returns (output * scale_range,
        lidar_correct * scale_range), net.py:3893, each [B,H,W]."""
        return self._run(input_lidar, input_rgb.detach())


class ResNet18LightImage(ResNet18Image):
    """net.py's ResNet18_NO_BN_l2_light_image (net.py:3895-4426) for inference: the image-guided network at 64 channels on every
    level, the variant for full KITTI frames.  weights: {layer name: (kernel, bias)} under the reference's attribute names
    (layer_shapes_resnet18_light_image), as Keras stores them.  Beside the narrower layers it differs from ResNet18Image in
    this: conv1_pre, a linear 3x3 layer, folds the stems into lidar_conv_total, 64 channels; conv1a and conv1a_extra read
    [image | lidar_conv_total]; lidar_conv_total is max-pooled by 2, 4 and 8 and concatenated BEHIND tensor_2_total,
    tensor_3_total and tensor_4, and those 128-wide tensors feed the next level and the skip concats; the last concat is
    [upsample_1 | lidar_conv_total].

    Here conv1_pre writes the channels 64 .. 127 of the [image | total] tensor, and ONE dtfill_max_pool_pyramid call reads them
    there and writes the upper halves of the three levels' wide tensors, whose lower halves conv2d, conv3d and conv4d write: the
    three pools cost one pass over the full-resolution tensor.  Called as net(input_lidar, input_rgb); H and W multiples of 8;
    detached, no host synchronisation, no activation buffer allocated after the first call at a shape, the returned tensors are
    the instance's own: as ResNet18Image."""

    NAME = "ResNet18_NO_BN_l2_light_image"
    WIDTHS, PRE, POOLS, LIDAR_SKIP = (LIGHT_WIDTH,) * 4, "conv1_pre", LIGHT_POOLS, True


def layer_shapes_resnet18(scale_num=4, if_correct=True):
    """{layer name: (ksize, Cin, Cout)} of the layers ResNet18_NO_BN_l2's forward uses (net.py:262-400), under the reference's
    attribute names.  The layers of RESNET_STRIDE2 have stride 2; those of RESNET_TRANSPOSED are Conv2DTranspose(Cout, 3,
    strides=2), whose Keras kernel is [3,3,Cout,Cin]; upsample_1 is an ordinary convolution, as in the reference."""
    return ResNet18.layer_shapes(scale_num, if_correct)


def layer_shapes_resnet18_image(scale_num=4, if_correct=True):
    """{layer name: (ksize, Cin, Cout)} of the layers ResNet18_NO_BN_l2_image's forward uses (net.py:3383-3893): those of
    layer_shapes_resnet18 and img_conv, the layer that reads the image, whose 64 channels stand in front of the stems, so the
    three layers that read that tensor are 64 channels wider."""
    return ResNet18Image.layer_shapes(scale_num, if_correct)


def layer_shapes_resnet18_light_image(scale_num=4, if_correct=True):
    """{layer name: (ksize, Cin, Cout)} of the layers ResNet18_NO_BN_l2_light_image's forward uses (net.py:3895-4426): 64 channels
    on every level.  conv1_pre folds the stems into 64 channels; conv1a and conv1a_extra read [image | conv1_pre]; the layers
    that read a level's tensor concatenated with a pooled conv1_pre output (conv3a, conv4a, their _extra, upsample_4) read 128
    channels, and the two _post layers whose skip tensor is such a concat read 192."""
    return ResNet18LightImage.layer_shapes(scale_num, if_correct)


def glorot_weights_resnet18(seed, scale_num=4, if_correct=True, bias=0.0):
    """glorot_weights() for ResNet18: float32 numpy arrays of Keras' shapes, [3,3,Cout,Cin] for the transposed layers."""
    return _glorot(layer_shapes_resnet18, seed, scale_num, if_correct, bias)


def glorot_weights_resnet18_image(seed, scale_num=4, if_correct=True, bias=0.0):
    """glorot_weights() for ResNet18Image: float32 numpy arrays of Keras' shapes, [3,3,Cout,Cin] for the transposed layers."""
    return _glorot(layer_shapes_resnet18_image, seed, scale_num, if_correct, bias)


def glorot_weights_resnet18_light_image(seed, scale_num=4, if_correct=True, bias=0.0):
    """glorot_weights() for ResNet18LightImage: float32 numpy arrays of Keras' shapes, [3,3,Cout,Cin] for the transposed layers."""
    return _glorot(layer_shapes_resnet18_light_image, seed, scale_num, if_correct, bias)


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

    This class holds the tape trunk of every ResNet, _run, driven by INFERENCE's facts (_ResNet).  Every float32 gradient sum
    the tape makes has exactly two terms, so the order in which the autograd engine runs the nodes cannot change a bit:
    - The base tensor (the stems; with an image the [image | lidar part] concat, IMAGE_WIDTH channels wider) and tensor_k_total
      for k = 1..3 (with POOLS, the wide tensors of levels 2 and 3) have three consumers: conv(k+1)a, conv(k+1)a_extra and a
      skip concat.  The two convolutions read ONE identity view, so the tensor's gradient is (d conv_a + d conv_a_extra) +
      d concat.  With LIDAR_SKIP the base tensor has the two convolutions only.
    - With POOLS the lidar part, PRE's output, has three consumers, the image concat, the pools and the last concat: the first
      two read one identity view, and the pools are ONE operator whose backward sums its levels in a fixed grouping, so the
      tensor's gradient is (d concat_image + d pools) + d concat_1.
    - img_conv reads the channels 0 .. IMAGE_WIDTH - 1 of the base tensor's gradient in place and stem k the channels behind
      (torch.cat's backward hands out slices, autograd's convolutions read them at an offset).
    No host synchronisation in either direction; activations are new tensors of each call.

    precision is an attribute of the instance, not an argument of the constructor (whose signature is every trainable
    network's): model.precision = "bf16", at any time between two steps; anything but "float32" or "bf16" raises ValueError
    there.  "float32", the default, is the fixed-order float32 chain in every layer and every gradient.  "bf16" is mixed
    precision for the layers that go through _wide and _up, forward (the bits of the inference class under precision="bf16")
    and backward (dtfill_conv2d_strided_backward_data_bf16 and its siblings): operands rounded to bf16 in registers, float32
    accumulation.  The head, the stems, img_conv, the pools, conv_output, the loss and KerasAdam stay float32; activations
    and gradients are float32 in memory; the parameters and the optimizer state are float32 master copies, packed anew inside
    every call.  No loss scaling is needed: bf16 has float32's exponent range and g stays float32 in memory, so a small
    gradient does not underflow on its way down as it would in float16."""

    INFERENCE = ResNet18
    _precision = "float32"

    @property
    def precision(self):
        return self._precision

    @precision.setter
    def precision(self, precision):
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s, got %r" % (PRECISIONS, precision))
        self._precision = precision

    def _wide(self, x, name, stride=1, residual=None, act="leaky"):
        from . import autograd

        layer = getattr(self, name)
        return autograd.conv2d_strided(x, layer.kernel, layer.bias, stride, residual, act, LEAKY_ALPHA, self.precision)

    def _up(self, x, name):
        from . import autograd

        layer = getattr(self, name)
        return autograd.conv2d_transpose(x, layer.kernel, layer.bias, "leaky", LEAKY_ALPHA, self.precision)

    def forward(self, input_lidar):
        """input_lidar: contiguous float32 CUDA tensor [B,H,W] in metres, H and W multiples of 8, a constant.  Returns two
        [B,H,W] tensors."""
        return self._run(input_lidar, None)

    def _run(self, input_lidar, rgb):
        from . import autograd

        facts = self.INFERENCE
        x = _checked_lidar(input_lidar)
        B, H, W = x.shape
        if facts.IMAGE_WIDTH:
            _check_rgb(rgb, x)
        with torch.cuda.device(x.device):
            correct, lidar = self._head(x)
            if facts.PRE:
                lidar = self._wide(lidar, facts.PRE, act="linear")  # lidar_conv_total, net.py:4220
            part, pooled = lidar, {}
            if facts.POOLS:
                part = lidar.view_as(lidar)  # ONE consumer of it for the image concat and the pools; the last concat is the other
                pooled = dict(zip(facts.POOLS, autograd.max_pool_pyramid(part, facts.POOLS)))  # factor -> the pool behind its level
            base = part
            if facts.IMAGE_WIDTH:  # net.py:3645-3649, 4222
                image = autograd.conv2d_image(rgb, self.img_conv.kernel, self.img_conv.bias, "leaky", LEAKY_ALPHA)
                base = torch.cat([image, part], dim=3)
            below, totals = base, []
            for k in range(4):  # net.py:551-674, 4224-4355
                name, stride = "conv%d" % (k + 1), 1 if k == 0 else 2
                both = below.view_as(below)  # ONE consumer of `below` for the two convolutions; the skip concat is the other
                t = self._wide(both, name + "a", stride)
                add = self._wide(both, name + "a_extra", stride, act="linear")
                total = self._wide(t, name + "b", residual=add)
                t = self._wide(total, name + "c")
                below = self._wide(t, name + "d", residual=total if k < 3 else None)
                if 1 << k in pooled:
                    below = torch.cat([below, pooled[1 << k]], dim=3)
                totals.append(below)
            for n in (4, 3, 2):  # net.py:680-724, 4360-4404
                up = torch.cat([self._up(below, "upsample_%d" % n), totals[n - 2]], dim=3)
                below = self._wide(up, "upsample_%d_post" % n)
            # net.py:728-742, 4408-4422: the whole base tensor, or lidar_conv_total itself (not the view the pools read)
            up = torch.cat([self._wide(below, "upsample_1"), lidar if facts.LIDAR_SKIP else base], dim=3)
            t = self._wide(up, "upsample_1_post")
            output = self._conv(t, "conv_output", "linear").view(B, H, W)
            return output * self._scale, correct * self._scale


class ResNet18ImageTrainable(ResNet18Trainable):
    """net.py's ResNet18_NO_BN_l2_image under a tape: ResNet18Image as a torch.nn.Module, ResNet18Trainable with img_conv
    (autograd.conv2d_image) in front of the stems.  weights: as ResNet18Image takes them; the parameters are <layer>.kernel and
    <layer>.bias, img_conv's among them.  forward(input_lidar, input_rgb) returns the bits ResNet18Image returns for the same
    weights.  input_rgb is a constant: the image is data, img_conv has no data gradient, and an input_rgb that requires a
    gradient raises ValueError.  The tensor with three consumers at level 1 is now the [image | stems] concat, 64 + 16 scale_num
    wide: two-term sums as before (ResNet18Trainable)."""

    INFERENCE = ResNet18Image

    def forward(self, input_lidar, input_rgb):
        """input_lidar: [B,H,W] in metres, H and W multiples of 8; input_rgb: contiguous float32 CUDA tensor [B,H,W,3]; both
        constants.  Returns two [B,H,W] tensors."""
        if input_rgb.requires_grad:
            raise ValueError("input_rgb is a constant: the image is data and img_conv has no data gradient; pass input_rgb.detach()")
        return self._run(input_lidar, input_rgb)


class ResNet18LightImageTrainable(ResNet18ImageTrainable):
    """net.py's ResNet18_NO_BN_l2_light_image under a tape: ResNet18LightImage as a torch.nn.Module over the same operators as
    ResNet18ImageTrainable and autograd.max_pool_pyramid.  weights: as ResNet18LightImage takes them; the parameters are
    <layer>.kernel and <layer>.bias in Keras' layouts.  forward(input_lidar, input_rgb) returns the bits ResNet18LightImage
    returns for the same weights; input_rgb is a constant.  Every float32 gradient sum of the tape has two terms: lidar_conv_total
    and the 128-wide tensors of levels 2 and 3 are grouped as ResNet18Trainable states under POOLS."""

    INFERENCE = ResNet18LightImage
