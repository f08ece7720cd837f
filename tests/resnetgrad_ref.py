"""The gradient of train.py:240-251's loss with respect to every variable of ResNet18_NO_BN_l2 (solution_DeepNet/net.py:458-745)
in numpy, for the tests only: resnet_ref's graph with every activation kept, then the chain rule composed of conv2b_ref (the wide,
strided and transposed layers' dx, dw, db and dresidual in their fixed orders), convb_ref (the layers with one input or one output
channel), gmc_grad_ref (the multi-channel fill's transpose) and loss_ref.  The head's forward and backward are netgrad_ref's
statements for SparsityCNN's head, the same lines of the reference, restated here from the stems' gradient on because
netgrad_ref.backward starts at SparsityCNN's own trunk.  The product does not import this file.

Where a tensor has more than one consumer its gradient is a float32 sum, and a sum of three terms depends on its grouping.  Four
tensors have three consumers: the stems (conv1a, conv1a_extra, the concat in front of upsample_1_post) and tensor_k_total for
k = 1..3 (conv(k+1)a, conv(k+1)a_extra, the concat of level k).  The grouping is (d conv_a + d conv_a_extra) + d concat: the two
convolutions are one consumer.  CONSUMERS states it; backward() builds every sum from it.  lidar_correct under joint_train is
netgrad_ref's: (stem + window steps) + output.  The reference's kernel_regularizer adds nothing: train.py:253 differentiates
total_loss alone.
"""
import numpy as np

import conv2_ref as C2
import conv2b_ref as RW
import conv_ref as C
import gmc_grad_ref
import loss_ref
import net_ref
import netgrad_ref
import resnet_ref

F = np.float32
ALPHA = net_ref.ALPHA
WIDTHS = resnet_ref.WIDTHS
# tensor -> its consumers, nested as its gradient is summed: a tuple is one two-term sum
CONSUMERS = {"stems": (("conv1a", "conv1a_extra"), "concat_1")}
CONSUMERS.update({"tensor_%d_total" % k: (("conv%da" % (k + 1), "conv%da_extra" % (k + 1)), "concat_%d" % (k + 1)) for k in (1, 2, 3)})


def _add(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, F) + np.asarray(b, F)).astype(F)


def forward(x, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4):
    """resnet_ref.forward with a tape: dict(output, correct, mask, lidars, tape: {layer: [(input, output, act, stride, residual)
    per call]}).  The head is netgrad_ref.forward's, statement by statement."""
    x = np.asarray(x, F)
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

    below, totals = stems, []
    for level in (1, 2, 3, 4):
        name, stride = "conv%d" % level, 1 if level == 1 else 2
        t = wide(below, name + "a", stride)
        add = wide(below, name + "a_extra", stride, act=C.LINEAR)
        total = wide(t, name + "b", residual=add)
        t = wide(total, name + "c")
        below = wide(t, name + "d", residual=total if level < 4 else None)
        totals.append(below)
    for level in (4, 3, 2):
        below = wide(np.concatenate([up(below, "upsample_%d" % level), totals[level - 2]], axis=-1), "upsample_%d_post" % level)
    t = wide(np.concatenate([wide(below, "upsample_1"), stems], axis=-1), "upsample_1_post")
    kernel, bias = weights["conv_output"]
    y = C.conv_ref(t, kernel, bias, C.LINEAR, ALPHA)
    tape["conv_output"] = [(t, y, C.LINEAR)]
    return dict(output=y[..., 0] * F(scale_range), correct=correct * F(scale_range), mask=mask, lidars=lidars, tape=tape, stems=stems)


def _wide_backward(weights, name, call, dy, grads, want_dx=True):
    """One wide layer: (dw, db) into grads[name]; returns (dx or None, dresidual or None)."""
    x, y, act, stride, has_residual = call
    kernel = weights[name][0]
    dy = np.ascontiguousarray(dy, F)
    grads[name] = RW.strided_dw_ref(x, dy, y, kernel.shape[0], stride, act, ALPHA)
    dx = RW.strided_dx_ref(dy, y, kernel, stride, act, ALPHA) if want_dx else None
    return dx, (RW.g_ref(dy, y, act, ALPHA) if has_residual else None)


def _up_backward(weights, name, call, dy, grads):
    """One Conv2DTranspose: the kernel's gradient in Keras' layout [3,3,Cout,Cin]; returns dx."""
    x, y, act = call
    dy = np.ascontiguousarray(dy, F)
    dw, db = RW.transpose_dw_ref(x, dy, y, act, ALPHA)
    grads[name] = (np.ascontiguousarray(dw.transpose(0, 1, 3, 2)), db)
    return RW.transpose_dx_ref(dy, y, C2.pack(weights[name][0]), act, ALPHA)


def backward_trunk(fw, weights, g_output, scale_range=90.0):
    """From the gradient of the first result down to the stems' concat: ({layer: (dw, db)} of every layer behind the stems, the
    gradient of the stems [B,H,W,16 scale_num]).  It does not depend on joint_train: the expensive part, worked out once."""
    tape, grads = fw["tape"], {}
    scale = F(scale_range)
    concat = {}  # level -> the gradient its concat sends to the skip tensor
    dy = netgrad_ref._layer_backward(weights, "conv_output", tape["conv_output"][0], (g_output * scale)[..., None], grads)
    dy, _ = _wide_backward(weights, "upsample_1_post", tape["upsample_1_post"][0], dy, grads)
    concat[1] = dy[..., 64:]
    dy, _ = _wide_backward(weights, "upsample_1", tape["upsample_1"][0], dy[..., :64], grads)
    for level in (2, 3, 4):
        width = WIDTHS[level - 2]
        dy, _ = _wide_backward(weights, "upsample_%d_post" % level, tape["upsample_%d_post" % level][0], dy, grads)
        concat[level] = dy[..., width:]
        dy = _up_backward(weights, "upsample_%d" % level, tape["upsample_%d" % level][0], dy[..., :width], grads)
    for level in (4, 3, 2, 1):  # dy: the gradient of tensor_<level>_total (level 4: of tensor_4)
        name = "conv%d" % level
        d_t, d_total = _wide_backward(weights, name + "d", tape[name + "d"][0], dy, grads)
        d_c, _ = _wide_backward(weights, name + "c", tape[name + "c"][0], d_t, grads)
        d_total = d_c if d_total is None else _add(d_c, d_total)  # conv c and conv d's residual: two terms
        d_t, d_add = _wide_backward(weights, name + "b", tape[name + "b"][0], d_total, grads)
        d_a, _ = _wide_backward(weights, name + "a", tape[name + "a"][0], d_t, grads)
        d_e, _ = _wide_backward(weights, name + "a_extra", tape[name + "a_extra"][0], d_add, grads)
        dy = _add(_add(d_a, d_e), concat[level])  # CONSUMERS: (conv_a + conv_a_extra) + concat
    return grads, dy


def backward(fw, weights, g_output, g_correct, table_size=7, if_correct=True, scale_range=90.0, scale_num=4, joint_train=False,
             trunk=None):
    """fw: forward()'s; g_output, g_correct: the gradients of its two results (None: unused); trunk: backward_trunk()'s result
    where it is shared between two settings of joint_train.  Returns {layer: (dw, db)} in Keras' layouts for every layer that
    receives a gradient."""
    tape, grads = fw["tape"], {}
    scale = F(scale_range)
    joint_train = joint_train and if_correct
    g_fill = None
    if g_output is not None:
        trunk_grads, dy = trunk if trunk is not None else backward_trunk(fw, weights, g_output, scale_range)
        grads.update(trunk_grads)
        names = net_ref.stem_names(scale_num)
        gs = [None] * 4
        for k in range(scale_num - 1, -1, -1):  # as netgrad_ref.backward from here on
            call = tape[names[k]][k // 3]
            dx = netgrad_ref._layer_backward(weights, names[k], call, np.ascontiguousarray(dy[..., 16 * k:16 * k + 16]), grads, joint_train)
            gs[k] = None if dx is None else dx[..., 0]
        if joint_train:
            if scale_num > 1:
                steps = gmc_grad_ref.backward(fw["mask"], fw["lidars"][1] if scale_num >= 3 else None,
                                              fw["lidars"][2] if scale_num == 4 else None, table_size, scale_num, [None] + gs[1:])
                g_fill = gs[0] + steps
            else:
                g_fill = gs[0]
    if not if_correct:
        return grads
    g_out2 = None if g_correct is None else g_correct * scale
    if g_fill is None and g_out2 is None:
        return grads
    g = g_out2 if g_fill is None else g_fill if g_out2 is None else g_fill + g_out2
    dy = (g * fw["mask"])[..., None]
    for name in ("correct_4",) + netgrad_ref.BRANCH[::-1]:
        dy = netgrad_ref._layer_backward(weights, name, tape[name][0], dy, grads, name != "correct_1")
    return grads


def loss_gradients(x, gt, weights, correct=True, **settings):
    """The step of train.py:232-253 on ResNet18_NO_BN_l2: forward, total = main + aux, the gradient of total with respect to
    every variable.  settings: table_size, if_correct, scale_range, scale_num, joint_train (a tuple of settings gives a dict
    of results that share the forward and everything behind the stems).  Returns ({layer: (dw, db)}, forward()'s dict, stats)."""
    joint = settings.pop("joint_train", False)
    fw = forward(x, weights, **settings)
    x, gt = np.asarray(x, F), np.asarray(gt, F)
    stats, _ = loss_ref.forward(fw["output"], gt, x if correct else None, fw["correct"] if correct else None)
    g_pred, g_corr = loss_ref.backward(fw["output"], gt, stats, F(1), F(1) if correct else None, x if correct else None,
                                       fw["correct"] if correct else None)
    if not isinstance(joint, tuple):
        return backward(fw, weights, g_pred, g_corr, joint_train=joint, **settings), fw, stats
    trunk = backward_trunk(fw, weights, g_pred, settings.get("scale_range", 90.0))  # joint_train a tuple: a dict per setting
    return {j: backward(fw, weights, g_pred, g_corr, joint_train=j, trunk=trunk, **settings) for j in joint}, fw, stats
