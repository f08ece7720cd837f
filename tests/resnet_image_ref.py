"""ResNet18_NO_BN_l2_image.call (solution_DeepNet/net.py:3383-3893) in numpy, for the tests only: the forward with a tape and
the gradient of train.py:240-251's loss with respect to every variable.  The reference's class is ResNet18_NO_BN_l2 line for
line but for img_conv on input_rgb, whose leaky output is concatenated in front of the stems, so this file is composed of
resnet_ref's, resnetgrad_ref's, netgrad_ref's, conv_ref's and convb_ref's functions: only the wiring is restated, with the
64-channel shift of every slice of the [image | stems] tensor.  The product does not import this file.

resnetgrad_ref.backward_trunk takes the tape as it is: it cuts the concat in front of upsample_1_post behind its first 64
channels, whatever the width of the rest, and returns the gradient of the tensor conv1a reads, here 64 + 16 scale_num wide and
summed as (d conv1a + d conv1a_extra) + d concat.  Its channels 0 .. 63 are img_conv's dy; the rest, handed to
resnetgrad_ref.backward as the trunk's result, are the stems' and go on into the head as there.  There is no gradient for the
image.
"""
import numpy as np

import conv_ref as C
import convb_ref as RB
import loss_ref
import net_ref
import netgrad_ref
import resnet_ref
import resnetgrad_ref as RG

F = np.float32
ALPHA = net_ref.ALPHA
IMAGE_WIDTH = 64


def layer_shapes(scale_num=4, if_correct=True):
    """{layer: (ksize, Cin, Cout)} from the reference's constructor (net.py:3391-3560): Keras infers Cin from the input, so
    the numbers are those of the tensors call() builds."""
    n = scale_num
    shapes = {}
    if if_correct:
        shapes.update(correct_1=(7, 1, 16), correct_2=(5, 16, 16), correct_3=(3, 16, 16), correct_4=(3, 16, 1))
    shapes["img_conv"] = (3, 3, 64)
    for name in net_ref.stem_names(n):
        shapes[name] = (3, 1, 16)
    below = 64 + 16 * n
    for level, width in enumerate(resnet_ref.WIDTHS, 1):
        for suffix, k, cin in (("a", 3, below), ("b", 3, width), ("a_extra", 1, below), ("c", 3, width), ("d", 3, width)):
            shapes["conv%d%s" % (level, suffix)] = (k, cin, width)
        below = width
    shapes.update(upsample_4=(3, 512, 256), upsample_4_post=(3, 512, 256), upsample_3=(3, 256, 128), upsample_3_post=(3, 256, 128),
                  upsample_2=(3, 128, 64), upsample_2_post=(3, 128, 64), upsample_1=(3, 64, 64), upsample_1_post=(3, 128 + 16 * n, 64),
                  conv_output=(1, 64, 1))
    return shapes


def plain_weights(weights, scale_num):
    """The weights of ResNet18_NO_BN_l2 that the image network's are with the image cut out: no img_conv, and the kernels of the
    three layers that read [image | stems] without the image's 64 input rows."""
    out = {k: v for k, v in weights.items() if k != "img_conv"}
    for name in ("conv1a", "conv1a_extra"):
        kernel, bias = weights[name]
        out[name] = (np.ascontiguousarray(kernel[:, :, IMAGE_WIDTH:]), bias)
    kernel, bias = weights["upsample_1_post"]  # reads [upsample_1 | image | stems]
    out["upsample_1_post"] = (np.ascontiguousarray(np.concatenate([kernel[:, :, :64], kernel[:, :, 64 + IMAGE_WIDTH:]], axis=2)), bias)
    return out


def forward(x, rgb, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4):
    """x float32 [B,H,W], rgb float32 [B,H,W,3] -> resnetgrad_ref.forward's dict: output, correct, mask, lidars, stems (here
    [image | stems]) and the tape."""
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
    kernel, bias = weights["img_conv"]
    image = C.conv_ref(rgb, kernel, bias, C.LEAKY, ALPHA)
    tape["img_conv"] = [(rgb, image, C.LEAKY)]
    stems = [image]  # net.py:3645-3649: tf.concat([img_conv_1, lidar_conv_total])
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

    below, totals = stems, []
    for level in (1, 2, 3, 4):  # net.py:3683-3806
        name, stride = "conv%d" % level, 1 if level == 1 else 2
        t = wide(below, name + "a", stride)
        add = wide(below, name + "a_extra", stride, act=C.LINEAR)
        total = wide(t, name + "b", residual=add)
        t = wide(total, name + "c")
        below = wide(t, name + "d", residual=total if level < 4 else None)
        totals.append(below)
    for level in (4, 3, 2):  # net.py:3812-3856
        below = wide(np.concatenate([up(below, "upsample_%d" % level), totals[level - 2]], axis=-1), "upsample_%d_post" % level)
    t = wide(np.concatenate([wide(below, "upsample_1"), stems], axis=-1), "upsample_1_post")  # net.py:3860-3890
    kernel, bias = weights["conv_output"]
    y = C.conv_ref(t, kernel, bias, C.LINEAR, ALPHA)
    tape["conv_output"] = [(t, y, C.LINEAR)]
    return dict(output=y[..., 0] * F(scale_range), correct=correct * F(scale_range), mask=mask, lidars=lidars, tape=tape, stems=stems)


def backward_trunk(fw, weights, g_output, scale_range=90.0):
    """resnetgrad_ref.backward_trunk on this tape: ({layer: (dw, db)} behind [image | stems], that tensor's gradient)."""
    return RG.backward_trunk(fw, weights, g_output, scale_range)


def backward(fw, weights, g_output, g_correct, table_size=7, if_correct=True, scale_range=90.0, scale_num=4, joint_train=False, trunk=None):
    """As resnetgrad_ref.backward.  Returns {layer: (dw, db)} in Keras' layouts for every layer that receives a gradient."""
    grads, shifted = {}, None
    if g_output is not None:
        trunk_grads, dy = trunk if trunk is not None else backward_trunk(fw, weights, g_output, scale_range)
        rgb, image, act = fw["tape"]["img_conv"][0]
        grads["img_conv"] = RB.dw_ref(rgb, np.ascontiguousarray(dy[..., :IMAGE_WIDTH]), image, weights["img_conv"][0].shape[0], act, ALPHA)
        shifted = (trunk_grads, np.ascontiguousarray(dy[..., IMAGE_WIDTH:]))  # stem k: 64 + 16 k on
    grads.update(RG.backward(fw, weights, g_output, g_correct, table_size, if_correct, scale_range, scale_num, joint_train, shifted))
    return grads


def loss_gradients(x, rgb, gt, weights, correct=True, **settings):
    """The step of train.py:232-253 on ResNet18_NO_BN_l2_image, as resnetgrad_ref.loss_gradients: joint_train a tuple gives a
    dict of results that share the forward and everything behind [image | stems]."""
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
