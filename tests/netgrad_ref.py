"""The gradient of train.py:240-251's loss with respect to every variable of SparsityCNN (solution_DeepNet/net.py:125-242) in
numpy, for the tests only: net_ref's forward with every activation kept, then the chain rule composed of convb_ref (the
convolutions' dx, dw and db in their fixed orders), gmc_grad_ref (the multi-channel fill's transpose) and loss_ref (the two
losses' gradients), with the elementwise steps as single float32 operations.  Written from the reference and the contracts in
include/dtfill.h; the product does not import this file.

Where a tensor has more than one consumer its gradient is a float32 sum, and a sum of three terms depends on its grouping.
There is one such tensor, lidar_correct under joint_train: the fill's input (consumed by the window steps, and as lidar_1 by
the first stem) and the network's second output.  The grouping is (stem + window steps) + output: the fill's input is one
consumer of lidar_correct, the second output the other.  lidar_conv_extra_1 is called on lidar_2 and on lidar_4; its
gradient is the sum of the two calls' (two terms: the order does not matter).
"""
import numpy as np

import conv_ref as C
import convb_ref as CB
import gmc_grad_ref
import loss_ref
import net_ref

F = np.float32
ALPHA = net_ref.ALPHA
TRUNK = ("conv1a", "conv1b", "conv1c", "conv1d")
BRANCH = ("correct_1", "correct_2", "correct_3")


def _chain(x, weights, names, acts, tape):
    """The layers `names` in sequence from x; every layer's (input, output) goes on the tape."""
    for name, act in zip(names, acts):
        kernel, bias = weights[name]
        y = C.conv_ref(x, kernel, bias, act, ALPHA)
        tape[name] = [(x, y, act)]
        x = y
    return x


def forward(x, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4):
    """net_ref.forward with a tape: dict(output, correct: the two results; mask; lidars; tape: {layer: [(input, output, act)
    per call]})."""
    x = np.asarray(x, F)
    tape = {}
    mask = (x > F(0.1)).astype(F)
    scaled = x / F(scale_range)
    if if_correct:
        t = _chain(scaled[..., None], weights, BRANCH + ("correct_4",), (C.LEAKY,) * 3 + (C.LINEAR,), tape)
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
    t = _chain(np.concatenate(stems, axis=-1), weights, TRUNK + ("conv_output",), (C.LEAKY,) * 4 + (C.LINEAR,), tape)
    return dict(output=t[..., 0] * F(scale_range), correct=correct * F(scale_range), mask=mask, lidars=lidars, tape=tape)


def _layer_backward(weights, name, call, dy, grads, want_dx=True):
    """One call of a layer: adds its (dw, db) to grads[name] and returns dx (None unless asked for)."""
    x, y, act = call
    dw, db = CB.dw_ref(x, dy, y, weights[name][0].shape[0], act, ALPHA)
    grads[name] = (dw, db) if name not in grads else (grads[name][0] + dw, grads[name][1] + db)
    return CB.dx_ref(dy, y, weights[name][0], act, ALPHA) if want_dx else None


def backward(fw, weights, g_output, g_correct, table_size=7, if_correct=True, scale_range=90.0, scale_num=4, joint_train=False):
    """fw: forward()'s; g_output, g_correct: the gradients of its two results (None: unused).  Returns {layer: (dw, db)} for
    every layer that receives a gradient."""
    tape, grads = fw["tape"], {}
    scale = F(scale_range)
    g_fill = None  # the gradient of the fill's input
    joint_train = joint_train and if_correct  # (without the branch nothing in front of the fill is trained)
    if g_output is not None:
        dy = (g_output * scale)[..., None]
        for name in ("conv_output",) + TRUNK[::-1]:
            dy = _layer_backward(weights, name, tape[name][0], dy, grads)
        names = net_ref.stem_names(scale_num)
        gs = [None] * 4
        for k in range(scale_num - 1, -1, -1):
            call = tape[names[k]][k // 3]  # lidar_conv_extra_1's second call is lidar_4's
            dx = _layer_backward(weights, names[k], call, np.ascontiguousarray(dy[..., 16 * k:16 * k + 16]), grads, joint_train)
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
    for name in ("correct_4",) + BRANCH[::-1]:
        dy = _layer_backward(weights, name, tape[name][0], dy, grads, name != "correct_1")
    return grads


def loss_gradients(x, gt, weights, correct=True, **settings):
    """The step of train.py:232-253 on KITTI frames (no crop here): forward, total = main + aux (aux with `correct`, as the
    driver's --correct), and the gradient of total with respect to every variable.  settings: table_size, if_correct,
    scale_range, scale_num, joint_train.  Returns ({layer: (dw, db)}, forward()'s dict, stats)."""
    joint = settings.pop("joint_train", False)
    fw = forward(x, weights, **settings)
    x, gt = np.asarray(x, F), np.asarray(gt, F)
    stats, _ = loss_ref.forward(fw["output"], gt, x if correct else None, fw["correct"] if correct else None)
    g_pred, g_corr = loss_ref.backward(fw["output"], gt, stats, F(1), F(1) if correct else None, x if correct else None,
                                       fw["correct"] if correct else None)
    return backward(fw, weights, g_pred, g_corr, joint_train=joint, **settings), fw, stats
