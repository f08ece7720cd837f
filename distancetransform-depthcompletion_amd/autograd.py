"""generate_multi_channel() of the reference's models (solution_DeepNet/net.py:83-122) as a differentiable torch operator.

In the reference the windowed fill sits inside the trained graph: with if_correct its input is the output of four learned
convolutions (net.py:469-486), its outputs feed the encoder (net.py:489), and the gradient is cut only when joint_train is
off (net.py:491-496).  generate_multi_channel() here is that operator on CUDA tensors: forward by
dtfill_generate_multi_channel, backward by dtfill_generate_multi_channel_backward (include/dtfill.h states both).
Differentiable in `data` only, once: tf.equal / tf.cast / tf.greater give the mask no gradient, and there is no double
backward.  joint_train = False is the caller's .detach() on the input.
"""
import torch
from torch.autograd.function import once_differentiable

from . import device


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
