"""SparsityCNN without a device: the numpy statement of its forward (tests/net_ref.py) on what is peculiar to the reference
(net.py:206 reuses lidar_conv_extra_1 and never calls lidar_conv_extra_3), and the class's layer table and weight checks."""
import importlib

import numpy as np
import pytest

import conv_ref as C
import gmc_ref
import net_ref

F = np.float32


@pytest.fixture(scope="module")
def net(pkg):
    return importlib.import_module(pkg.__name__ + ".net")


@pytest.fixture(scope="module")
def frames(pkg):
    synth = importlib.import_module(pkg.__name__ + ".synth")
    return synth.kitti_iid(2, p=0.08, seed=3, hw=(9, 12))


def test_stem_four_follows_extra_1_and_extra_3_is_never_read(net, frames):
    weights = net.glorot_weights(1, scale_num=4, if_correct=False, bias=0.1)
    want = net_ref.forward(frames, weights, if_correct=False)
    assert want["stems"].shape == frames.shape + (64,)
    # channels 48..63 are lidar_conv_extra_1 applied to lidar_4
    scaled = (frames / F(90.0)) * (frames > F(0.1))
    lidar_4 = net_ref.fills(scaled.astype(F), (frames > F(0.1)).astype(F), 7, 4)[3]
    kernel, bias = weights["lidar_conv_extra_1"]
    C.assert_same(want["stems"][..., 48:], C.conv_ref(lidar_4[..., None], kernel, bias, C.LEAKY, 0.2), "stem 4")
    other = dict(weights, lidar_conv_extra_1=net.glorot_weights(2, bias=0.1)["lidar_conv_extra_1"])
    changed = net_ref.forward(frames, other, if_correct=False)["stems"]
    assert (changed[..., 16:32] != want["stems"][..., 16:32]).any() and (changed[..., 48:] != want["stems"][..., 48:]).any()
    assert (changed[..., :16] == want["stems"][..., :16]).all() and (changed[..., 32:48] == want["stems"][..., 32:48]).all()
    # NaN weights in lidar_conv_extra_3 change nothing
    nan = dict(weights, lidar_conv_extra_3=(np.full((3, 3, 1, 16), np.nan, F), np.full(16, np.nan, F)))
    got = net_ref.forward(frames, nan, if_correct=False)
    assert all((got[k].view(np.uint32) == want[k].view(np.uint32)).all() for k in ("output", "correct", "stems"))
    assert net.stem_layers(4) == tuple(net_ref.stem_names(4)) and "lidar_conv_extra_3" not in net.layer_shapes(4, True)
    net.SparsityCNN(nan, if_correct=False)  # accepted, ignored
    assert "lidar_conv_extra_3" not in net.SparsityCNN(nan, if_correct=False)._host


def test_fill_step_is_gmc_refs_step_in_float32_tap_order(frames):
    """net_ref's float32 tap-order sum against gmc_ref's float64 one: the same bits where one tap is selected, within
    gmc_ref's bound elsewhere."""
    data = (frames / F(90.0)).astype(F)
    mask = (frames > F(0.1)).astype(F)
    several = 0
    for _ in range(3):
        out, cnt, abs_sum = gmc_ref.gmc_step(data, mask, 7)
        got = net_ref.fill_step(data, mask, 7)
        gmc_ref.assert_step_matches(got, out, cnt, abs_sum, "fill_step")
        several += int(((cnt > 1) & (abs_sum > 0)).sum())
        data, mask = got, gmc_ref.next_mask(got)
    assert several > 0  # (the case the two sums can differ in is there)


@pytest.mark.parametrize("if_correct", (True, False))
@pytest.mark.parametrize("scale_num", (1, 2, 3, 4))
def test_channel_counts(net, scale_num, if_correct):
    shapes = net.layer_shapes(scale_num, if_correct)
    assert shapes["conv1a"] == (7, 16 * scale_num, 16) and shapes["conv_output"] == (1, 16, 1)
    assert ("correct_1" in shapes) == if_correct and (shapes.get("correct_4") == (3, 16, 1)) == if_correct
    assert len(net.stem_layers(scale_num)) == scale_num
    assert [n for n in ("lidar_conv_extra_1", "lidar_conv_extra_2") if n in shapes] == ["lidar_conv_extra_1", "lidar_conv_extra_2"][:max(scale_num - 1, 0)]
    layers = {(k, cin, cout) for k, cin, cout in shapes.values()}
    assert layers <= {l[:3] for l in C.NET_LAYERS}  # every layer is one the conv tests cover
    weights = net.glorot_weights(0, scale_num, if_correct, bias=0.1)
    assert {n: (k.shape, b.shape) for n, (k, b) in weights.items() if n in shapes} == \
        {n: ((k, k, cin, cout), (cout,)) for n, (k, cin, cout) in shapes.items()}
    assert ("lidar_conv_extra_3" in weights) == (scale_num == 4)
    assert all(k.dtype == F and b.dtype == F and np.abs(b).max() > 0 for k, b in weights.values())
    model = net.SparsityCNN(weights, if_correct=if_correct, scale_num=scale_num)
    assert set(model._host) == set(shapes)
    x = np.zeros((1, 3, 4), F)
    x[0, 1, 2] = 10
    out = net_ref.forward(x, weights, if_correct=if_correct, scale_num=scale_num)
    assert out["stems"].shape == (1, 3, 4, 16 * scale_num) and out["output"].shape == out["correct"].shape == (1, 3, 4)


def test_weight_dict_checks(net):
    weights = net.glorot_weights(0)
    for name in ("conv1a", "correct_2", "lidar_conv_extra_2", "conv_output"):
        with pytest.raises(ValueError, match=name):
            net.SparsityCNN({k: v for k, v in weights.items() if k != name})
    net.SparsityCNN({k: v for k, v in weights.items() if not k.startswith("correct")}, if_correct=False)
    kernel, bias = weights["conv1a"]
    for bad in ((kernel[..., :8], bias), (kernel, bias[:8]), (kernel.transpose(3, 2, 0, 1), bias), (kernel[:5, :5], bias),
                (kernel[:, :, :32], bias)):
        with pytest.raises(ValueError, match="conv1a"):
            net.SparsityCNN(dict(weights, conv1a=bad))
    with pytest.raises(ValueError, match="conv1a"):
        net.SparsityCNN(weights, scale_num=2)  # conv1a of a scale_num 4 net reads 64 channels, not 32
    with pytest.raises(ValueError, match="conv9z"):
        net.SparsityCNN(dict(weights, conv9z=weights["conv1b"]))
    for bad in (dict(scale_num=0), dict(scale_num=5), dict(table_size=6), dict(scale_range=0.0), dict(scale_range=float("inf"))):
        with pytest.raises(ValueError):
            net.SparsityCNN(weights, **bad)
    import torch

    with pytest.raises(ValueError):
        net.SparsityCNN(weights)(torch.zeros((1, 4, 4)))  # a host tensor
