"""SparsityCNN.call (solution_DeepNet/net.py:125-242) in numpy, for the tests only: the convolutions are conv_ref's chains, the
multi-channel fill is gmc_ref's selection rule, and the elementwise steps are single float32 operations.  Written from the reference;
the product does not import this file.

gmc_ref.gmc_step sums a window's selected taps in float64 and rounds once, which holds the device's bits only where one tap is
selected; fill_step here sums them in float32 in tap order, the order include/dtfill.h fixes, and tests/test_net.py holds it to
gmc_step within gmc_ref's bound.
"""
import numpy as np

import conv_ref as C
import gmc_ref

F = np.float32
ALPHA = 0.2  # tf.nn.leaky_relu's default


def stem_names(scale_num):
    """net.py:164-212: lidar_conv, extra_1, extra_2 and -- net.py:206 -- extra_1 again; extra_3 is never called."""
    return ["lidar_conv", "lidar_conv_extra_1", "lidar_conv_extra_2", "lidar_conv_extra_1"][:scale_num]


def _layer(x, weights, name, act):
    kernel, bias = weights[name]
    return C.conv_ref(x, kernel, bias, act, ALPHA)


def fill_step(data, mask, ts):
    """One step of generate_multi_channel (net.py:83-96) as include/dtfill.h states it: gmc_ref's selection, and the selected
    values summed in float32 in tap (row-major) order from +0, which fixes the bits where several taps are selected."""
    B, H, W = data.shape
    half = (ts - 1) // 2
    w = gmc_ref.weights(ts)
    pd = np.pad(data, ((0, 0), (half, half), (half, half)))
    pm = np.pad(mask, ((0, 0), (half, half), (half, half)))
    taps = [(i, j) for i in range(ts) for j in range(ts)]
    s = np.stack([pm[:, i:i + H, j:j + W] * w[i * ts + j] for i, j in taps], axis=-1)
    sel = s == s.max(axis=-1, keepdims=True)
    total = np.zeros((B, H, W), F)
    for k, (i, j) in enumerate(taps):
        total = total + np.where(sel[..., k], pd[:, i:i + H, j:j + W], F(0))
    return total / (F(0.000001) + sel.sum(axis=-1).astype(F))


def fills(data, mask, table_size, scale_num):
    """generate_multi_channel, net.py:83-122: [lidar_1 .. lidar_<scale_num>], each [B,H,W]."""
    out = [data]
    for _ in range(scale_num - 1):
        data = fill_step(data, mask, table_size)
        mask = gmc_ref.next_mask(data)
        out.append(data)
    return out


def forward(x, weights, table_size=7, if_correct=True, scale_range=90.0, scale_num=4):
    """x float32 [B,H,W] -> dict(output, correct: net.py:242's two results, [B,H,W]; stems: the concatenated stem tensor
    [B,H,W,16 scale_num])."""
    x = np.asarray(x, F)
    mask = (x > F(0.1)).astype(F)
    scaled = x / F(scale_range)
    if if_correct:
        t = _layer(scaled[..., None], weights, "correct_1", C.LEAKY)
        t = _layer(t, weights, "correct_2", C.LEAKY)
        t = _layer(t, weights, "correct_3", C.LEAKY)
        correct = _layer(t, weights, "correct_4", C.LINEAR)[..., 0]
    else:
        correct = scaled
    correct = correct * mask
    lidars = fills(correct, mask, table_size, scale_num)
    stems = np.concatenate([_layer(l[..., None], weights, n, C.LEAKY) for l, n in zip(lidars, stem_names(scale_num))], axis=-1)
    t = stems
    for name in ("conv1a", "conv1b", "conv1c", "conv1d"):
        t = _layer(t, weights, name, C.LEAKY)
    output = _layer(t, weights, "conv_output", C.LINEAR)[..., 0]
    return dict(output=output * F(scale_range), correct=correct * F(scale_range), stems=stems)
