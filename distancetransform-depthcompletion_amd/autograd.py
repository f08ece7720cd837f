"""The reference's in-graph pieces around the network as differentiable torch operators: generate_multi_channel() of its models
(solution_DeepNet/net.py:83-122), the objective of its training step (solution_DeepNet/train.py:210-251, train_loss below), and
the exact fill itself (tools.py:13-35, fill below), which the reference could only run in numpy outside the graph.

In the reference the windowed fill sits inside the trained graph: with if_correct its input is the output of four learned
convolutions (net.py:469-486), its outputs feed the encoder (net.py:489), and the gradient is cut only when joint_train is
off (net.py:491-496).  generate_multi_channel() here is that operator on CUDA tensors: forward by
dtfill_generate_multi_channel, backward by dtfill_generate_multi_channel_backward (include/dtfill.h states both).
Differentiable in `data` only, once: tf.equal / tf.cast / tf.greater give the mask no gradient, and there is no double
backward.  joint_train = False is the caller's .detach() on the input.

conv2d() is a layer of the network itself under the tape (dtfill_conv2d forward; dtfill_conv2d_backward_data and
dtfill_conv2d_backward_weights backward, both in fixed summation orders), and net.SparsityCNNTrainable is net.py's SparsityCNN
composed of it, of generate_multi_channel() and of single torch operations: with train_loss() that is train.py:232-254's step.
conv2d_strided() and conv2d_transpose() are the wide layers of ResNet18_NO_BN_l2 under the tape (dtfill_conv2d_strided and
dtfill_conv2d_transpose forward; their _backward_data and _backward_weights entry points backward), and net.ResNet18Trainable is
the paper's network composed of them.

Threads and streams: every operator here may be called from several host threads on one stream and on several streams at once.
The cached pieces (device.default_op's operator, the backward workspaces) are per stream, and one call's launches are enqueued
under that piece's lock, so they stay contiguous on their stream; the outputs are the call's own tensors.  No lock is held
across a host synchronisation: there is none.
"""
import torch
from torch.autograd.function import once_differentiable

from . import device
from .conv import PRECISIONS, _backward_data, _backward_weights, _forward, _forward_bf16, pack_bf16_device


class _WindowSteps(torch.autograd.Function):
    """lidar_2 .. lidar_scale_num from (data, mask); lidar_1 is data itself and stays outside."""

    @staticmethod
    def forward(ctx, data, mask, table_size, scale_num):
        outs = device.generate_multi_channel_device(data, mask, table_size, scale_num)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None: a NULL gradient
        ctx.table_size, ctx.scale_num = table_size, scale_num
        # the backward reads the masks, never the data: out2 / out3 only where a later step's mask derives from them
        ctx.save_for_backward(mask, outs[1] if scale_num >= 3 else None, outs[2] if scale_num == 4 else None)
        return tuple(outs[1:scale_num])

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        if not ctx.needs_input_grad[0] or all(g is None for g in grads):
            return None, None, None, None
        mask, out2, out3 = ctx.saved_tensors
        gs = [None] + [None if g is None else g.contiguous() for g in grads] + [None] * (3 - len(grads))
        grad = device.generate_multi_channel_backward_device(mask, out2, out3, gs, ctx.table_size, ctx.scale_num)
        return grad, None, None, None


def generate_multi_channel(data, mask, table_size=7, scale_num=4):
    """data, mask: contiguous float32 CUDA tensors [B,H,W].  Returns (lidar_1, lidar_2, lidar_3, lidar_4) with None beyond
    scale_num, like the reference; lidar_1 is `data` itself, so its gradient flows through ordinary autograd."""
    if scale_num not in (1, 2, 3, 4):
        raise ValueError("scale_num must be 1, 2, 3 or 4, got %r" % (scale_num,))
    if scale_num == 1:
        device.generate_multi_channel_device(data, mask, table_size, 1)  # (the argument checks)
        return (data, None, None, None)
    steps = _WindowSteps.apply(data, mask.detach(), int(table_size), int(scale_num))
    return (data,) + tuple(steps) + (None,) * (4 - scale_num)


class _TrainLoss(torch.autograd.Function):
    """(main, aux) of train.py:240-249 as 0-d float32 tensors; aux only with a correction."""

    @staticmethod
    def forward(ctx, pred, correction, gt, lidar, cfg):
        stats = device.train_loss_device(pred, gt, lidar, correction, **cfg)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None: nothing is computed for it
        ctx.cfg = cfg
        ctx.save_for_backward(pred, correction, gt, lidar, stats)
        # fresh tensors, not two views of one: the caller may go on in place (total = main; total += aux)
        main = stats[0].to(torch.float32)
        return (main, stats[1].to(torch.float32)) if correction is not None else (main,)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_main, g_aux=None):
        pred, correction, gt, lidar, stats = ctx.saved_tensors
        want_pred = ctx.needs_input_grad[0] and g_main is not None
        want_corr = ctx.needs_input_grad[1] and g_aux is not None
        if not (want_pred or want_corr):
            return None, None, None, None, None
        scalar = lambda g: None if g is None else g.to(torch.float32).contiguous()
        # pred's gradient needs neither the correction nor the LiDAR; they ride along only where the correction's is asked for
        grad_pred, grad_corr = device.train_loss_backward_device(
            pred, gt, stats, scalar(g_main), scalar(g_aux), lidar if want_corr else None, correction if want_corr else None,
            want_pred=want_pred, want_correction=want_corr, **ctx.cfg)
        return grad_pred, grad_corr, None, None, None


def train_loss(pred, gt, lidar=None, correction=None, dataset="KITTI", gt_thr=None, in_thr=None, rows=None, cols=None):
    """train.py:215-249 on contiguous float32 CUDA tensors [B,H,W]: pred = depth_predicted, correction = lidar_correction (with
    --correct, together with lidar), gt and lidar the loader's frames after the driver's row crop.  dataset and the overrides
    as device.train_loss_device.  Returns (main, aux), 0-d float32 tensors, aux None without a correction; train.py:251's
    total = main + aux is the caller's add, so autograd splits the upstream gradient by itself.  Differentiable in pred and
    correction only, once; an unused output costs nothing in the backward; no host synchronisation in either direction."""
    cfg = dict(dataset=dataset, gt_thr=gt_thr, in_thr=in_thr, rows=rows, cols=cols)
    lidar = None if lidar is None else lidar.detach()
    out = _TrainLoss.apply(pred, correction, gt.detach(), lidar, cfg)
    return (out[0], out[1]) if correction is not None else (out[0], None)


class _Fill(torch.autograd.Function):
    """(depth, dt, index, status) of DtFill.run in tensors of the call's own; depth alone carries a gradient."""

    @staticmethod
    def forward(ctx, x, src_thr, val_thr, metric):
        with torch.cuda.device(x.device):
            op = device.default_op(metric)
        B = x.shape[0] if x.dim() == 3 else 0  # (run raises for anything but [B,H,W])
        # the operator's own buffers are overwritten by its next call: these are not
        out = dict(depth=torch.empty_like(x), dt=torch.empty_like(x), index=torch.empty_like(x, dtype=torch.int32),
                   status=torch.empty((B,), dtype=torch.int32, device=x.device))
        op.run(x, src_thr, val_thr, out=out)
        ctx.set_materialize_grads(False)  # an unused depth arrives as None: nothing is launched for it
        ctx.val_thr = val_thr
        ctx.save_for_backward(x, out["index"])
        ctx.mark_non_differentiable(out["dt"], out["index"], out["status"])
        return out["depth"], out["dt"], out["index"], out["status"]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_depth, g_dt=None, g_index=None, g_status=None):
        if g_depth is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        x, index = ctx.saved_tensors
        grad_x, _ = device.fill_backward_device(x, index, g_depth.to(torch.float32).contiguous(), ctx.val_thr)
        return grad_x, None, None, None


def fill(x, src_thr=0.1, val_thr=0.1, metric="l1_cv"):
    """The exact fill depth = depth_list[lbl - 1] (tools.py:13-35, eval_NYU.py:120-133) as a differentiable operator, for the place
    where net.py:155 has the windowed generate_multi_channel behind the learned correction of net.py:136-153.  x: contiguous
    float32 CUDA tensor [B,H,W].  Returns (depth, dt, index, status) as DtFill.run gives them, in tensors of their own.
    Differentiable in x through depth only, once; dt, index and status are marked non-differentiable.  The predicates and the
    labels are constants of the differentiation: the backward (include/dtfill.h, dtfill_fill_backward) sends the gradient of
    every pixel that read depth_list[k] to the k-th valued pixel, bitwise reproducibly; a frame whose status carries
    _lib.FRAME_INDEX_ERROR gets a zero gradient.  With depth unused nothing is launched in the backward; no host
    synchronisation in either direction.  The depth epilogue (row crop, floor) and outlier_removal stay out: they compose as
    torch ops, or as this package's device functions on a detached input, on either side."""
    return _Fill.apply(x, float(src_thr), float(val_thr), metric)


class _FillValues(torch.autograd.Function):
    """(filled, dt, index, pixel, status) of DtFill.run(x) and the nearest gather of values; filled alone carries a gradient,
    and only to values."""

    @staticmethod
    def forward(ctx, x, values, src_thr, metric):
        with torch.cuda.device(x.device):
            op = device.default_op(metric)
        # the operator's own buffers are overwritten by its next call: these are not
        out = dict(dt=torch.empty_like(x), index=torch.empty_like(x, dtype=torch.int32))
        op.run(x, src_thr, 0.1, want=("dt", "index"), out=out)
        filled, pixel, status = device.nearest_gather_device(x, out["index"], values, src_thr)
        ctx.set_materialize_grads(False)  # an unused filled arrives as None: nothing is launched for it
        ctx.src_thr = src_thr
        ctx.save_for_backward(x, out["index"])
        ctx.mark_non_differentiable(out["dt"], out["index"], pixel, status)
        return filled, out["dt"], out["index"], pixel, status

    @staticmethod
    @once_differentiable
    def backward(ctx, g_filled, g_dt=None, g_index=None, g_pixel=None, g_status=None):
        if g_filled is None or not ctx.needs_input_grad[1]:
            return None, None, None, None
        x, index = ctx.saved_tensors
        grad_values, _ = device.nearest_gather_backward_device(x, index, g_filled.to(torch.float32).contiguous(), ctx.src_thr)
        return None, grad_values, None, None


def fill_values(x, values, src_thr=0.1, metric="l1_cv"):
    """The exact fill with the sources decided by one tensor and the payload read from another: every pixel of `filled` holds
    `values` at the pixel's nearest source of x (include/dtfill.h, dtfill_nearest_gather).  This is the exact fill for the place
    where net.py:131-155 has the windowed one: there the mask comes from the raw LiDAR, valued_mask = input_lidar > 0.1, and the
    values from the learned correction lidar_correct, so the recipe is
        filled, dt, index, pixel, status = fill_values(input_lidar, lidar_correct)
    A pixel of x is a source iff NOT((1.0f - x) > src_thr) in float32 (DtFill's source predicate: with src_thr = 0.1 that is
    x above about 0.9, or NaN, where the reference's mask is x > 0.1; the two agree on LiDAR in metres, whose returns lie beyond 1 m).
    x: contiguous float32 CUDA tensor [B,H,W], a constant; values: [B,C,H,W] with 1 <= C <= 64, or [B,H,W] as C = 1 (filled
    then comes back [B,H,W]).  Returns (filled, dt, index, pixel, status): dt and index as DtFill.run(x) gives them, pixel int32
    [B,H,W] the flat pixel row*W + col of the nearest source (-1 in a frame without one, where filled is +0.0), status the
    gather's (_lib.FRAME_NO_SOURCE, _lib.FRAME_INDEX_ERROR), all in tensors of the call's own.  Differentiable in values through
    filled only, once; dt, index, pixel and status are marked non-differentiable.  The backward (dtfill_nearest_gather_backward)
    sends the gradient of every pixel to the source it read, bitwise reproducibly; with filled unused nothing is launched.  No
    host synchronisation in either direction."""
    squeeze = values.dim() == 3
    out = _FillValues.apply(x.detach(), values.unsqueeze(1) if squeeze else values, float(src_thr), metric)
    return (out[0].squeeze(1) if squeeze else out[0],) + tuple(out[1:])


class _Unproject(torch.autograd.Function):
    """(points, counts, pixel, status) of device.unproject_device; points alone carries a gradient, to x and to payload."""

    @staticmethod
    def forward(ctx, x, payload, K, E, val_thr, capacity):
        points, counts, status, _, pixel = device.unproject_device(x, K, E, val_thr, payload, capacity)
        ctx.set_materialize_grads(False)  # unused points arrive as None: nothing is launched for them
        ctx.hw = tuple(x.shape[1:])
        ctx.save_for_backward(pixel, counts, K, E)
        ctx.mark_non_differentiable(counts, pixel, status)
        return points, counts, pixel, status

    @staticmethod
    @once_differentiable
    def backward(ctx, g_points, g_counts=None, g_pixel=None, g_status=None):
        want_x, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_points is None or not (want_x or want_p):
            return None, None, None, None, None, None
        pixel, counts, K, E = ctx.saved_tensors
        grad_x, grad_payload, _ = device.unproject_backward_device(g_points.to(torch.float32).contiguous(), pixel, counts, K, E,
                                                                   ctx.hw, want_payload=want_p)
        return (grad_x if want_x else None), grad_payload, None, None, None, None


def unproject(x, K, E, val_thr=0.1, payload=None, capacity=None):
    """Depth frames to ordered point clouds as a differentiable operator (include/dtfill.h, dtfill_unproject): the step from a
    completed depth map to the pseudo-LiDAR cloud a 3D consumer trains on.  x: contiguous float32 CUDA tensor [B,H,W]; K
    [3,3] or [B,3,3], E [4,4] or [B,4,4] (numpy or tensors, constants); payload: like x, carried as each record's fourth
    float; capacity: records per frame (default H*W).  Returns (points [B,N,3 or 4], counts int32 [B,2], pixel int32 [B,N],
    status int32 [B]) as device.unproject_device gives them, in tensors of the call's own.  Differentiable in x and payload
    through points, once: the validity mask is a constant of the differentiation and the map is affine in the depth, so the
    backward (dtfill_unproject_backward) is a scatter of one value per record, bitwise reproducible; the records beyond
    counts[b, 0] are not written and take no gradient.  counts, pixel and status are marked non-differentiable.  No host
    synchronisation in either direction; every buffer is the call's own, allocated under the stream it runs on."""
    device._check_tensor(x, "x")
    B = x.shape[0]
    Kd = device._calibration(K, 3, B, x.device, "K")
    Ed = device._calibration(E, 4, B, x.device, "E")
    return _Unproject.apply(x, payload, Kd, Ed, float(val_thr), capacity)


def _channel_slice(g):
    """g [B,H,W,C] as (tensor, offset): g itself at 0 if it is contiguous; the wider contiguous tensor it is a channel slice of
    (what torch.cat's backward hands out) and its first channel there, read in place; else a contiguous copy at 0."""
    g = g.to(torch.float32)
    if g.is_contiguous() or g.dim() != 4:
        return g.contiguous(), 0
    B, H, W, C = g.shape
    wide = g.stride(2)
    if g.stride(3) == 1 and wide > C and g.stride(1) == W * wide and g.stride(0) == H * W * wide:
        offset = g.storage_offset() % wide
        start = g.storage_offset() - offset
        if offset + C <= wide and start + B * H * W * wide <= g.untyped_storage().nbytes() // 4:
            return g.as_strided((B, H, W, wide), (H * W * wide, W * wide, wide, 1), start), offset
    return g.contiguous(), 0


class _Conv(torch.autograd.Function):
    """y of a convolution of `kind` (conv._KINDS: narrow, strided, transposed, image; w of a transposed one is the packed kernel
    [3,3,Cin,Cout]); the backward asks the library only for the gradients that are needed.  Both through conv.py's cores."""

    @staticmethod
    def forward(ctx, kind, x, w, bias, residual, stride, act, alpha, precision="float32"):
        if precision == "bf16":  # w is packed for this call; the float32 x, w and y are what the backward reads
            y = _forward_bf16(kind, x, pack_bf16_device(w, kind == "transposed"), bias, stride, residual, act, alpha, None, 0)
        else:
            y = _forward(kind, x, w, bias, stride, residual, act, alpha, None, 0)
        ctx.set_materialize_grads(False)  # an unused y arrives as None: nothing is launched for it
        ctx.kind, ctx.stride, ctx.act, ctx.alpha, ctx.precision = kind, stride, act, alpha, precision
        ctx.save_for_backward(x, w, None if act == "linear" else y)  # (a linear layer's derivative does not read y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y):
        want_x, want_w, want_b, want_r = ctx.needs_input_grad[1:5]
        if g_y is None or not (want_x or want_w or want_b or want_r):
            return (None,) * 9
        x, w, y = ctx.saved_tensors
        dy, at = _channel_slice(g_y)
        dx = dr = dw = db = None
        if want_x:
            dx = _backward_data(ctx.kind, dy, w, ctx.stride, y, ctx.act, ctx.alpha, at, 0, None, 0, want_r, ctx.precision)
            if want_r:
                dx, dr = dx
            dx = dx.view(x.shape)  # ([B,H,W,1] of a plane x)
        elif want_r:  # g alone: the compare and the one rounded product of the contract, as single torch operations
            g = dy[..., at:at + w.shape[3]]
            dr = (g if y is None else torch.where(y > 0, g, g * ctx.alpha)).contiguous()
        if want_w or want_b:
            dw, db = _backward_weights(ctx.kind, x, dy, w.shape[0], ctx.stride, y, ctx.act, ctx.alpha, at, 0, w.shape[3], want_b,
                                       ctx.precision)
        return None, dx, (dw if want_w else None), db, dr, None, None, None, None


class _MaxPoolPyramid(torch.autograd.Function):
    """The pooled tensors of `levels` from x by one forward call; the backward is one call too, with whichever gradients arrived."""

    @staticmethod
    def forward(ctx, x, levels):
        outs = device.max_pool_pyramid_device(x, levels)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None: a NULL dy
        ctx.levels = levels
        ctx.save_for_backward(x)  # the winners are found again from x: no argmax tensor is kept
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        if not ctx.needs_input_grad[0] or all(g is None for g in grads):
            return None, None
        (x,) = ctx.saved_tensors
        slices = [(None, 0) if g is None else _channel_slice(g) for g in grads]
        dx = device.max_pool_pyramid_backward_device(x, [t for t, _ in slices], ctx.levels, 0, x.shape[3], [at for _, at in slices])
        return dx, None


def max_pool_pyramid(x, levels=(2, 4, 8)):
    """tf.nn.max_pool of one tensor by every k of `levels` (2, 4, 8; ksize = strides = k, 'SAME') as one differentiable operator:
    the three pools net.py's ResNet18_NO_BN_l2_light_image takes of conv1_pre's output (net.py:4285, 4320, 4353).  x: contiguous
    float32 CUDA tensor [B,H,W,C], C a multiple of 4, H and W multiples of the largest level.  Returns a tuple of tensors
    [B,H/k,W/k,C] along `levels` by device.max_pool_pyramid_device (include/dtfill.h, dtfill_max_pool_pyramid): x is read once.
    Differentiable in x, once: the backward is ONE call of dtfill_max_pool_pyramid_backward with whichever gradients arrived
    (an unused output is a NULL dy), which finds the winners again from x and writes dx = (t_2 + t_4) + t_8 in that fixed
    grouping, so x receives one gradient from the three pools and every bit of it is a function of the inputs alone.  A gradient
    that is a channel slice of a wider contiguous tensor (torch.cat's backward) is read in place.  No host synchronisation in
    either direction."""
    return _MaxPoolPyramid.apply(x, tuple(int(k) for k in levels))


def _conv(kind, x, w, bias, residual, stride, act, alpha, precision="float32"):
    if not alpha >= 0:
        raise ValueError("alpha must be >= 0 (the derivative is taken by the sign of the output), got %r" % (alpha,))
    if precision not in PRECISIONS:
        raise ValueError("precision must be one of %s, got %r" % (PRECISIONS, precision))
    return _Conv.apply(kind, x, w, bias, residual, stride, act, float(alpha), precision)


def conv2d(x, w, bias=None, act="linear", alpha=0.2):
    """A stride-1 'same' float32 convolution with its activation as a differentiable operator: a layer of net.py's SparsityCNN
    under train.py:232-254's tape.  x: contiguous float32 CUDA tensor [B,H,W,Cin], or [B,H,W] for Cin = 1; w: [ksize,ksize,Cin,
    Cout], a Keras Conv2D.kernel as stored; bias: [Cout] or None; act: "linear" or "leaky" (y > 0 ? y : y * alpha, alpha >= 0).
    Returns y [B,H,W,Cout] by device.conv2d_device (include/dtfill.h, dtfill_conv2d).  Differentiable in x, w and bias, once:
    the backward calls dtfill_conv2d_backward_data for x and dtfill_conv2d_backward_weights for w and bias, each only where
    that gradient is needed, in their fixed summation orders, so every gradient bit is a function of the inputs and the shape
    alone.  A gradient of y that is a channel slice of a wider contiguous tensor (torch.cat's backward: a stem's 16 channels
    of conv1a's input gradient) is read in place, at dy_offset.  The shapes are dtfill_conv2d's domain (DtfillError otherwise).
    No host synchronisation in either direction; the workspace is the stream's cached one."""
    return _conv("narrow", x, w, bias, None, 1, act, alpha)


def conv2d_image(x, w, bias=None, act="linear", alpha=0.2):
    """The layer that reads the image as a differentiable operator: img_conv of net.py's ResNet18_NO_BN_l2_image under
    train.py:232-254's tape.  x: contiguous float32 CUDA tensor [B,H,W,Cin] with Cin 2, 3 or 4, a constant; w: [ksize,ksize,Cin,
    Cout], a Keras Conv2D.kernel as stored, Cout a multiple of 16; bias: [Cout] or None.  Returns y [B,H,W,Cout] by
    device.conv2d_image_device (include/dtfill.h, dtfill_conv2d_image).  Differentiable in w and bias, once, by
    dtfill_conv2d_image_backward_weights in its fixed two-level order; a gradient of y that is a channel slice of a wider
    contiguous tensor (torch.cat's backward) is read in place.  There is no gradient for x: the image is data, train.py:253
    differentiates with respect to the variables only, and the library has no such kernel; an x that requires a gradient
    raises ValueError rather than receiving none silently.  No host synchronisation in either direction."""
    if x.requires_grad:
        raise ValueError("conv2d_image has no gradient for x: the image is data (train.py:253 differentiates with respect to the "
                         "variables only); pass x.detach()")
    return _conv("image", x, w, bias, None, 1, act, alpha)


def conv2d_strided(x, w, bias=None, stride=1, residual=None, act="linear", alpha=0.2, precision="float32"):
    """A wide 'same' float32 convolution of stride 1 or 2 with its residual add and its activation as a differentiable operator:
    a layer of net.py's ResNet18_NO_BN_l2 under train.py:232-254's tape.  x: contiguous float32 CUDA tensor [B,H,W,Cin]; w:
    [ksize,ksize,Cin,Cout], a Keras Conv2D.kernel as stored; bias: [Cout] or None; residual: [B,Ho,Wo,Cout] or None, added in
    front of the activation.  Returns y by device.conv2d_strided_device (include/dtfill.h, dtfill_conv2d_strided).
    Differentiable in x, w, bias and residual, once: dtfill_conv2d_strided_backward_data gives the gradients of x and of the
    residual (g itself), dtfill_conv2d_strided_backward_weights those of w and bias, each only where it is needed, in their
    fixed summation orders.  A gradient of y that is a channel slice of a wider contiguous tensor (torch.cat's backward) is
    read in place.  The reference's kernel_regularizer takes no part: train.py:253 differentiates total_loss alone.  At
    stride 2 H and W must be even.  No host synchronisation in either direction.
    precision = "bf16" (ksize 1 or 3): the node packs w (dtfill_conv2d_pack_bf16), runs dtfill_conv2d_strided_bf16 and keeps
    the float32 x, w and y; its backward calls dtfill_conv2d_strided_backward_data_bf16 and _weights_bf16.  One tape node, the
    same tensors saved, the sliced gradient read in place and no host synchronisation, as under "float32"; the gradients are
    float32 tensors within the header's bounds and their bits are a function of the inputs and the shape alone.  Anything
    else than "float32" or "bf16" raises ValueError."""
    return _conv("strided", x, w, bias, residual, int(stride), act, alpha, precision)


def conv2d_transpose(x, kernel, bias=None, act="linear", alpha=0.2, precision="float32"):
    """tf.keras.layers.Conv2DTranspose(Cout, 3, strides=2, padding='same') with its activation as a differentiable operator.
    x: contiguous float32 CUDA tensor [B,H,W,Cin]; kernel: [3,3,Cout,Cin], the layer's kernel as Keras stores it; bias: [Cout]
    or None.  Returns y [B,2H,2W,Cout] by device.conv2d_transpose_device (include/dtfill.h, dtfill_conv2d_transpose).  The
    pack to the ABI's [3,3,Cin,Cout] is a permute inside the graph, so the kernel's gradient arrives in Keras' layout through
    autograd's own permute.  Differentiable in x, kernel and bias, once, by dtfill_conv2d_transpose_backward_data and _weights
    in their fixed summation orders.  No weight-decay term, as in conv2d_strided.  No host synchronisation.
    precision = "bf16": dtfill_conv2d_transpose_bf16 forward and dtfill_conv2d_transpose_backward_data_bf16 and _weights_bf16
    backward, as conv2d_strided states."""
    return _conv("transposed", x, kernel.permute(0, 1, 3, 2).contiguous(), bias, None, 2, act, alpha, precision)
