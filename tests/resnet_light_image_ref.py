"""ResNet18_NO_BN_l2_light_image.call (solution_DeepNet/net.py:4119-4425) in numpy, for the tests only: the forward with a tape and
the gradient of train.py:240-251's loss with respect to every variable, in the style of resnet_image_ref.py.  Composed of
resnetgrad_ref's, netgrad_ref's, resnet_ref's, conv_ref's and convb_ref's functions and pool_ref's: only the wiring is restated.
The product does not import this file.

Where a tensor has three consumers its gradient is grouped as the product's tape groups it.  lidar_conv_total, conv1_pre's
output: (d concat_image + d pools) + d concat_1, the pools' own sum being pool_ref.backward's (t_2 + t_4) + t_8.  The 128-wide
tensors of levels 2 and 3 and tensor_1_total: (d conv_a + d conv_a_extra) + d concat, as in resnetgrad_ref.
"""
import numpy as np

import conv_ref as C
import convb_ref as RB
import loss_ref
import net_ref
import netgrad_ref
import pool_ref
import resnet_ref
import resnetgrad_ref as RG

F = np.float32
ALPHA = net_ref.ALPHA
WIDTH = 64
POOLS = {2: 2, 3: 4, 4: 8}  # level -> the pool of lidar_conv_total concatenated behind its tensor


def layer_shapes(scale_num=4, if_correct=True):
    """{layer: (ksize, Cin, Cout)} from the reference's constructor (net.py:3911-4061): Keras infers Cin from the input, so the
    numbers are those of the tensors call() builds."""
    shapes = {}
    if if_correct:
        shapes.update(correct_1=(7, 1, 16), correct_2=(5, 16, 16), correct_3=(3, 16, 16), correct_4=(3, 16, 1))
    shapes["img_conv"] = (3, 3, 64)
    for name in net_ref.stem_names(scale_num):
        shapes[name] = (3, 1, 16)
    shapes["conv1_pre"] = (3, 16 * scale_num, 64)
    shapes.update(conv1a=(3, 128, 64), conv1a_extra=(1, 128, 64), conv2a=(3, 64, 64), conv2a_extra=(1, 64, 64),
                  conv3a=(3, 128, 64), conv3a_extra=(1, 128, 64), conv4a=(3, 128, 64), conv4a_extra=(1, 128, 64))
    for level in (1, 2, 3, 4):
        for suffix in "bcd":
            shapes["conv%d%s" % (level, suffix)] = (3, 64, 64)
    shapes.update(upsample_4=(3, 128, 64), upsample_3=(3, 64, 64), upsample_2=(3, 64, 64), upsample_4_post=(3, 192, 64),
                  upsample_3_post=(3, 192, 64), upsample_2_post=(3, 128, 64), upsample_1_post=(3, 128, 64), upsample_1=(3, 64, 64),
                  conv_output=(1, 64, 1))
    return shapes


def forward(x, rgb, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4):
    """x float32 [B,H,W], rgb float32 [B,H,W,3] -> resnetgrad_ref.forward's dict and total (lidar_conv_total), total1 ([image |
    total]) and pooled ({level: the 128-wide tensor of levels 2, 3, 4})."""
    x, rgb = np.asarray(x, F), np.asarray(rgb, F)
    tape = {}
    mask = (x > F(0.1)).astype(F)
    scaled = x / F(scale_range)
    if if_correct:
        t = netgrad_ref._chain(scaled[..., None], weights, netgrad_ref.BRANCH + ("correct_4",), (C.LEAKY,) * 3 + (C.LINEAR,), tape)
        correct = t[..., 0] * mask
    else:
        correct = scaled * mask
    lidars = net_ref.fills(correct, mask, table_size, scale_num)
    stems = []
    for lidar, name in zip(lidars, net_ref.stem_names(scale_num)):
        kernel, bias = weights[name]
        y = C.conv_ref(lidar[..., None], kernel, bias, C.LEAKY, ALPHA)
        tape.setdefault(name, []).append((lidar[..., None], y, C.LEAKY))
        stems.append(y)
    stems = np.concatenate(stems, axis=-1)

    def wide(v, name, stride=1, residual=None, act=C.LEAKY):
        y = resnet_ref._wide(v, weights, name, stride, residual, act)
        tape[name] = [(v, y, act, stride, residual is not None)]
        return y

    def up(v, name):
        y = resnet_ref._up(v, weights, name)
        tape[name] = [(v, y, C.LEAKY)]
        return y

    total = wide(stems, "conv1_pre", act=C.LINEAR)  # net.py:4220: no leaky_relu follows
    kernel, bias = weights["img_conv"]
    image = C.conv_ref(rgb, kernel, bias, C.LEAKY, ALPHA)
    tape["img_conv"] = [(rgb, image, C.LEAKY)]
    total1 = np.concatenate([image, total], axis=-1)  # net.py:4222
    below, totals, pooled = total1, [], {}
    for level in (1, 2, 3, 4):  # net.py:4224-4355
        name, stride = "conv%d" % level, 1 if level == 1 else 2
        t = wide(below, name + "a", stride)
        add = wide(below, name + "a_extra", stride, act=C.LINEAR)
        mid = wide(t, name + "b", residual=add)
        t = wide(mid, name + "c")
        below = wide(t, name + "d", residual=mid if level < 4 else None)
        if level > 1:
            below = pooled[level] = np.concatenate([below, pool_ref.max_pool(total, POOLS[level])], axis=-1)
        totals.append(below)
    for level in (4, 3, 2):  # net.py:4360-4404
        below = wide(np.concatenate([up(below, "upsample_%d" % level), totals[level - 2]], axis=-1), "upsample_%d_post" % level)
    t = wide(np.concatenate([wide(below, "upsample_1"), total], axis=-1), "upsample_1_post")  # net.py:4408-4420
    kernel, bias = weights["conv_output"]
    y = C.conv_ref(t, kernel, bias, C.LINEAR, ALPHA)
    tape["conv_output"] = [(t, y, C.LINEAR)]
    return dict(output=y[..., 0] * F(scale_range), correct=correct * F(scale_range), mask=mask, lidars=lidars, tape=tape, stems=stems,
                total=total, total1=total1, pooled=pooled)


def backward_trunk(fw, weights, g_output, scale_range=90.0):
    """From the gradient of the first result down to the stems' concat: ({layer: (dw, db)} of every layer behind the stems, the
    gradient of the stems [B,H,W,16 scale_num]).  It does not depend on joint_train."""
    tape, grads = fw["tape"], {}
    scale = F(scale_range)
    concat = {}  # level -> the gradient its skip concat sends to the level's tensor
    dy = netgrad_ref._layer_backward(weights, "conv_output", tape["conv_output"][0], (g_output * scale)[..., None], grads)
    dy, _ = RG._wide_backward(weights, "upsample_1_post", tape["upsample_1_post"][0], dy, grads)
    d_last = dy[..., WIDTH:]  # to lidar_conv_total, through the last concat
    dy, _ = RG._wide_backward(weights, "upsample_1", tape["upsample_1"][0], dy[..., :WIDTH], grads)
    for level in (2, 3, 4):
        dy, _ = RG._wide_backward(weights, "upsample_%d_post" % level, tape["upsample_%d_post" % level][0], dy, grads)
        concat[level - 1] = dy[..., WIDTH:]  # 64 wide at level 1, 128 at levels 2 and 3
        dy = RG._up_backward(weights, "upsample_%d" % level, tape["upsample_%d" % level][0], dy[..., :WIDTH], grads)
    d_pool = {}  # level -> the gradient of the pooled tensor behind it
    for level in (4, 3, 2, 1):  # dy: the gradient of the level's tensor, 128 wide at levels 2 .. 4
        name = "conv%d" % level
        if level > 1:
            d_pool[level], dy = dy[..., WIDTH:], dy[..., :WIDTH]
        d_t, d_mid = RG._wide_backward(weights, name + "d", tape[name + "d"][0], dy, grads)
        d_c, _ = RG._wide_backward(weights, name + "c", tape[name + "c"][0], d_t, grads)
        d_mid = d_c if d_mid is None else RG._add(d_c, d_mid)
        d_t, d_add = RG._wide_backward(weights, name + "b", tape[name + "b"][0], d_mid, grads)
        d_a, _ = RG._wide_backward(weights, name + "a", tape[name + "a"][0], d_t, grads)
        d_e, _ = RG._wide_backward(weights, name + "a_extra", tape[name + "a_extra"][0], d_add, grads)
        dy = RG._add(d_a, d_e)
        if level > 1:
            dy = RG._add(dy, concat[level - 1])  # (conv_a + conv_a_extra) + concat
    rgb, image, act = tape["img_conv"][0]  # dy: the gradient of [image | total]
    grads["img_conv"] = RB.dw_ref(rgb, np.ascontiguousarray(dy[..., :WIDTH]), image, weights["img_conv"][0].shape[0], act, ALPHA)
    d_pools = pool_ref.backward(fw["total"], [np.ascontiguousarray(d_pool[level]) for level in (2, 3, 4)])
    d_total = RG._add(RG._add(dy[..., WIDTH:], d_pools), d_last)  # (concat_image + pools) + concat_1
    d_stems, _ = RG._wide_backward(weights, "conv1_pre", tape["conv1_pre"][0], d_total, grads)
    return grads, d_stems


def backward(fw, weights, g_output, g_correct, table_size=7, if_correct=True, scale_range=90.0, scale_num=4, joint_train=False, trunk=None):
    """As resnetgrad_ref.backward, whose head this is.  Returns {layer: (dw, db)} in Keras' layouts."""
    if g_output is not None and trunk is None:
        trunk = backward_trunk(fw, weights, g_output, scale_range)
    return RG.backward(fw, weights, g_output, g_correct, table_size, if_correct, scale_range, scale_num, joint_train, trunk)


def loss_gradients(x, rgb, gt, weights, correct=True, **settings):
    """The step of train.py:232-253 on ResNet18_NO_BN_l2_light_image, as resnet_image_ref.loss_gradients: joint_train a tuple
    gives a dict of results that share the forward and everything behind the stems."""
    joint = settings.pop("joint_train", False)
    fw = forward(x, rgb, weights, **settings)
    x, gt = np.asarray(x, F), np.asarray(gt, F)
    stats, _ = loss_ref.forward(fw["output"], gt, x if correct else None, fw["correct"] if correct else None)
    g_pred, g_corr = loss_ref.backward(fw["output"], gt, stats, F(1), F(1) if correct else None, x if correct else None,
                                       fw["correct"] if correct else None)
    trunk = backward_trunk(fw, weights, g_pred, settings.get("scale_range", 90.0))
    joints = joint if isinstance(joint, tuple) else (joint,)
    out = {j: backward(fw, weights, g_pred, g_corr, joint_train=j, trunk=trunk, **settings) for j in joints}
    return (out if isinstance(joint, tuple) else out[joint]), fw, stats
