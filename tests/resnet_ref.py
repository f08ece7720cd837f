"""ResNet18_NO_BN_l2.call (solution_DeepNet/net.py:458-745) in numpy, for the tests only: net_ref's head, conv_ref's chains for
the layers with one input or one output channel, conv2_ref's for the wide, strided and transposed ones.  Written from the
reference; the product does not import this file.  forward64 is the same graph in float64 torch, for the bound of
tests/test_resnet.py.
"""
import numpy as np

import conv2_ref as C2
import conv_ref as C
import net_ref

F = np.float32
ALPHA = net_ref.ALPHA
WIDTHS = (64, 128, 256, 512)
TRANSPOSED = ("upsample_4", "upsample_3", "upsample_2")


def head(x, weights, table_size, if_correct, scale_range, scale_num):
    """net.py:464-547, the lines of SparsityCNN's head: (lidar_correct [B,H,W], the concatenated stems [B,H,W,16 scale_num])."""
    x = np.asarray(x, F)
    mask = (x > F(0.1)).astype(F)
    scaled = x / F(scale_range)
    if if_correct:
        t = net_ref._layer(scaled[..., None], weights, "correct_1", C.LEAKY)
        t = net_ref._layer(t, weights, "correct_2", C.LEAKY)
        t = net_ref._layer(t, weights, "correct_3", C.LEAKY)
        correct = net_ref._layer(t, weights, "correct_4", C.LINEAR)[..., 0]
    else:
        correct = scaled
    correct = correct * mask
    lidars = net_ref.fills(correct, mask, table_size, scale_num)
    stems = np.concatenate([net_ref._layer(l[..., None], weights, n, C.LEAKY)
                            for l, n in zip(lidars, net_ref.stem_names(scale_num))], axis=-1)
    return correct, stems


def _wide(x, weights, name, stride=1, residual=None, act=C.LEAKY):
    kernel, bias = weights[name]
    return C2.strided_ref(x, kernel, bias, stride, residual, act, ALPHA)


def _up(x, weights, name):
    kernel, bias = weights[name]  # Keras's [3,3,Cout,Cin]
    return C2.transpose_ref(x, C2.pack(kernel), bias, C.LEAKY, ALPHA)


def forward(x, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4):
    """x float32 [B,H,W], H and W multiples of 8 -> dict(output, correct: net.py:745's two results; stems)."""
    correct, stems = head(x, weights, table_size, if_correct, scale_range, scale_num)
    below, totals = stems, []
    for level in (1, 2, 3, 4):  # net.py:551-674
        name, stride = "conv%d" % level, 1 if level == 1 else 2
        t = _wide(below, weights, name + "a", stride)
        add = _wide(below, weights, name + "a_extra", stride, act=C.LINEAR)
        total = _wide(t, weights, name + "b", residual=add)
        t = _wide(total, weights, name + "c")
        below = _wide(t, weights, name + "d", residual=total if level < 4 else None)
        totals.append(below)
    for level in (4, 3, 2):  # net.py:680-724
        up = np.concatenate([_up(below, weights, "upsample_%d" % level), totals[level - 2]], axis=-1)
        below = _wide(up, weights, "upsample_%d_post" % level)
    up = np.concatenate([_wide(below, weights, "upsample_1"), stems], axis=-1)  # net.py:728-742
    t = _wide(up, weights, "upsample_1_post")
    output = net_ref._layer(t, weights, "conv_output", C.LINEAR)[..., 0]
    return dict(output=output * F(scale_range), correct=correct * F(scale_range), stems=stems)


def forward64(x, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4):
    """The same graph from the stems on in float64 torch, and a bound on |float32 forward - it| per output, composed from the
    per-layer bounds.  (The head is the float32 one: its fills select by equality, a float64 head would be another function.)
    A layer y = conv(v) + bias + residual of K = taps x Cin links, evaluated in float32, errs by at most
    d = gamma(K + 3) (conv(|v|, |w|) + |bias| + |residual|) per element on the inputs it is given: one rounding per link, bias
    add, residual add and leaky product.  To first order in those d the output moves by sum over layers of J d, J the
    Jacobian of the output with respect to the layer's y in the float64 graph, so |error| <= sum |J| d.  The bound returned is
    twice that: the factor covers the terms of second order and the elements that lie within their own error of leaky_relu's
    kink, where the slope the perturbed value meets differs from J's by at most 1 - alpha < 1 times the element's error.
    A worst-case bound through |w| alone, which needs no Jacobian, grows by the absolute row sum of every layer, about 50 here,
    and is vacuous after twenty-five of them.  Returns dict(output, bound, correct)."""
    import torch

    correct, stems = head(x, weights, table_size, if_correct, scale_range, scale_num)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    leaky = lambda y: torch.where(y > 0, y, y * float(F(ALPHA)))
    probes = []  # per layer: (a zero added to y, to differentiate by; d)

    def raw(y, kernel, stride, transposed):
        if transposed:  # Keras's [3,3,Cout,Cin]
            out = torch.nn.functional.conv_transpose2d(y, kernel.permute(3, 2, 0, 1), stride=2)
            return out[:, :, :2 * y.shape[2], :2 * y.shape[3]]
        k = kernel.shape[0]
        (_, pt, pb), (_, pl, pr) = C2.same_rule(y.shape[2], k, stride), C2.same_rule(y.shape[3], k, stride)
        return torch.nn.functional.conv2d(torch.nn.functional.pad(y, (pl, pr, pt, pb)), kernel.permute(3, 2, 0, 1), stride=stride)

    def layer(v, name, stride=1, residual=None, act=True):
        kernel, bias = (t64(a) for a in weights[name])
        transposed = name in TRANSPOSED
        K = (4 if transposed else kernel.shape[0] ** 2) * v.shape[1]
        b = bias.view(1, -1, 1, 1)
        y = raw(v, kernel, stride, transposed) + b
        with torch.no_grad():
            scale = raw(v.abs(), kernel.abs(), stride, transposed) + b.abs() + (0 if residual is None else residual.abs())
        if residual is not None:
            y = y + residual
        probe = torch.zeros_like(y, requires_grad=True)
        probes.append((probe, C.gamma(K + 3) * scale))
        y = y + probe
        return leaky(y) if act else y

    s = t64(stems).permute(0, 3, 1, 2)
    below, totals = s, []
    for level in (1, 2, 3, 4):
        name, stride = "conv%d" % level, 1 if level == 1 else 2
        t = layer(below, name + "a", stride)
        total = layer(t, name + "b", residual=layer(below, name + "a_extra", stride, act=False))
        below = layer(layer(total, name + "c"), name + "d", residual=total if level < 4 else None)
        totals.append(below)
    for level in (4, 3, 2):
        below = layer(torch.cat([layer(below, "upsample_%d" % level), totals[level - 2]], 1), "upsample_%d_post" % level)
    t = layer(torch.cat([layer(below, "upsample_1"), s], 1), "upsample_1_post")
    out = layer(t, "conv_output", act=False)[:, 0]
    flat, first_order = out.reshape(-1), []
    for p in range(flat.numel()):
        grads = torch.autograd.grad(flat[p], [probe for probe, _ in probes], retain_graph=True)
        first_order.append(sum(float((g.abs() * d).sum()) for g, (_, d) in zip(grads, probes)))
    out = out.detach().numpy()
    r = np.float64(F(scale_range))  # the last product: one more rounding
    bound = 2 * np.array(first_order).reshape(out.shape) * r + C.gamma(1) * np.abs(out) * r
    return dict(output=out * r, bound=bound, correct=correct * F(scale_range))
