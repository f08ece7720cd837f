"""ResNet18 (ResNet18_NO_BN_l2, solution_DeepNet/net.py:245-745) without a device: the class's layer table against the
constructor's numbers, its weight checks, and the numpy statement of its forward (tests/resnet_ref.py) against a float64 torch
forward of the same graph."""
import importlib

import numpy as np
import pytest

import conv_ref as C
import resnet_ref

F = np.float32


@pytest.fixture(scope="module")
def net(pkg):
    return importlib.import_module(pkg.__name__ + ".net")


@pytest.fixture(scope="module")
def frames(pkg):
    return importlib.import_module(pkg.__name__ + ".synth").kitti_iid(1, p=0.2, seed=20, hw=(8, 16))


# net.py:262-400, typed out: (ksize, Cin, Cout); Cin of conv1a, conv1a_extra and upsample_1_post at scale_num 4
CONSTRUCTOR = dict(
    correct_1=(7, 1, 16), correct_2=(5, 16, 16), correct_3=(3, 16, 16), correct_4=(3, 16, 1),
    lidar_conv=(3, 1, 16), lidar_conv_extra_1=(3, 1, 16), lidar_conv_extra_2=(3, 1, 16),
    conv1a=(3, 64, 64), conv1b=(3, 64, 64), conv1a_extra=(1, 64, 64), conv1c=(3, 64, 64), conv1d=(3, 64, 64),
    conv2a=(3, 64, 128), conv2b=(3, 128, 128), conv2a_extra=(1, 64, 128), conv2c=(3, 128, 128), conv2d=(3, 128, 128),
    conv3a=(3, 128, 256), conv3b=(3, 256, 256), conv3a_extra=(1, 128, 256), conv3c=(3, 256, 256), conv3d=(3, 256, 256),
    conv4a=(3, 256, 512), conv4b=(3, 512, 512), conv4a_extra=(1, 256, 512), conv4c=(3, 512, 512), conv4d=(3, 512, 512),
    upsample_4=(3, 512, 256), upsample_4_post=(3, 512, 256), upsample_3=(3, 256, 128), upsample_3_post=(3, 256, 128),
    upsample_2=(3, 128, 64), upsample_2_post=(3, 128, 64), upsample_1=(3, 64, 64), upsample_1_post=(3, 128, 64),
    conv_output=(1, 64, 1))


def test_layer_shapes_against_the_constructor(net):
    assert net.layer_shapes_resnet18(4, True) == CONSTRUCTOR
    assert net.RESNET_STRIDE2 == ("conv2a", "conv2a_extra", "conv3a", "conv3a_extra", "conv4a", "conv4a_extra")
    assert net.RESNET_TRANSPOSED == ("upsample_4", "upsample_3", "upsample_2") == resnet_ref.TRANSPOSED
    assert net.RESNET_WIDTHS == resnet_ref.WIDTHS == (64, 128, 256, 512)
    for scale_num in (1, 2, 3, 4):
        for if_correct in (True, False):
            shapes = net.layer_shapes_resnet18(scale_num, if_correct)
            assert shapes["conv1a"] == (3, 16 * scale_num, 64) and shapes["conv1a_extra"] == (1, 16 * scale_num, 64)
            assert shapes["upsample_1_post"] == (3, 64 + 16 * scale_num, 64)
            assert ("correct_1" in shapes) == if_correct and "lidar_conv_extra_3" not in shapes
            assert len(shapes) == len(CONSTRUCTOR) - (0 if if_correct else 4) - (3 - min(scale_num, 3))
            # every layer goes to an entry point that takes it: one channel in or out to dtfill_conv2d, the others wide
            for name, (k, cin, cout) in shapes.items():
                assert (cin == 1 and cout == 16) or (cout == 1 and cin in (16, 64)) or (cin % 16 == 0 and cout % 16 == 0), name
            weights = net.glorot_weights_resnet18(0, scale_num, if_correct, bias=0.1)
            assert ("lidar_conv_extra_3" in weights) == (scale_num == 4)
            for name, (k, cin, cout) in shapes.items():
                kernel, bias = weights[name]
                want = (k, k, cout, cin) if name in net.RESNET_TRANSPOSED else (k, k, cin, cout)  # Keras's layouts
                assert kernel.shape == want and bias.shape == (cout,) and kernel.dtype == bias.dtype == F, name
            model = net.ResNet18(weights, if_correct=if_correct, scale_num=scale_num)
            assert set(model._host) == set(shapes)
            assert all(model._host[n][0].shape == (3, 3) + shapes[n][1:] for n in net.RESNET_TRANSPOSED)  # packed once, here


def test_weight_dict_checks(net):
    weights = net.glorot_weights_resnet18(0)
    for name in ("conv1a", "conv3a_extra", "upsample_4", "upsample_1_post", "correct_2", "lidar_conv_extra_2", "conv_output"):
        with pytest.raises(ValueError, match=name):
            net.ResNet18({k: v for k, v in weights.items() if k != name})
    net.ResNet18({k: v for k, v in weights.items() if not k.startswith("correct")}, if_correct=False)
    kernel, bias = weights["upsample_4"]  # Keras's [3,3,256,512]
    for bad in ((kernel.transpose(0, 1, 3, 2), bias), (kernel, bias[:8]), (kernel[:, :, :128], bias)):
        with pytest.raises(ValueError, match="upsample_4"):
            net.ResNet18(dict(weights, upsample_4=bad))
    with pytest.raises(ValueError, match="conv1a"):
        net.ResNet18(weights, scale_num=2)  # conv1a of a scale_num 4 net reads 64 channels, not 32
    with pytest.raises(ValueError, match="conv9z"):
        net.ResNet18(dict(weights, conv9z=weights["conv1b"]))
    with pytest.raises(ValueError, match="ResNet18_NO_BN_l2"):
        net.ResNet18(dict(weights, conv5a=weights["conv1b"]))
    with pytest.raises(ValueError, match="SparsityCNN"):
        net.SparsityCNN(dict(net.glorot_weights(0), conv2a=weights["conv2a"]))  # a ResNet layer is none of SparsityCNN's
    for bad in (dict(scale_num=0), dict(scale_num=5), dict(table_size=6), dict(scale_range=0.0), dict(scale_range=float("inf"))):
        with pytest.raises(ValueError):
            net.ResNet18(weights, **bad)
    import torch

    with pytest.raises(ValueError):
        net.ResNet18(weights)(torch.zeros((1, 8, 8)))  # a host tensor


def test_frames_must_be_multiples_of_8(net):
    """Refused before any device work, so a host tensor shows it."""
    import torch

    model = net.ResNet18(net.glorot_weights_resnet18(0, 1, False), if_correct=False, scale_num=1)
    for H, W in ((12, 16), (8, 20), (7, 8), (16, 9)):
        with pytest.raises(ValueError, match="multiples of 8"):
            model(torch.zeros((1, H, W)))


def test_stem_four_follows_extra_1_and_extra_3_is_never_read(net, frames):
    weights = net.glorot_weights_resnet18(1, 4, False, bias=0.1)
    _, stems = resnet_ref.head(frames, weights, 7, False, 90.0, 4)
    other = dict(weights, lidar_conv_extra_1=net.glorot_weights_resnet18(2, bias=0.1)["lidar_conv_extra_1"])
    _, changed = resnet_ref.head(frames, other, 7, False, 90.0, 4)
    assert (changed[..., 16:32] != stems[..., 16:32]).any() and (changed[..., 48:] != stems[..., 48:]).any()
    assert (changed[..., :16] == stems[..., :16]).all() and (changed[..., 32:48] == stems[..., 32:48]).all()
    nan = dict(weights, lidar_conv_extra_3=(np.full((3, 3, 1, 16), np.nan, F), np.full(16, np.nan, F)))
    assert (resnet_ref.head(frames, nan, 7, False, 90.0, 4)[1].view(np.uint32) == stems.view(np.uint32)).all()
    assert "lidar_conv_extra_3" not in net.ResNet18(nan, if_correct=False)._host  # accepted, ignored
    assert net.stem_layers(4)[3] == "lidar_conv_extra_1"


def test_numpy_forward_against_float64(net, frames):
    """resnet_ref.forward against the float64 torch forward of the same graph on a 1 x 8 x 16 frame (level 4 is 1 x 2 pixels),
    within resnet_ref.forward64's bound, whose derivation is its docstring: twice the first-order sum over the layers of
    |Jacobian of the output| times the layer's gamma_(K+3) (sum |x| |w| + |bias| + |residual|), plus the last product's rounding."""
    weights = net.glorot_weights_resnet18(7, 4, True, bias=0.1)
    got = resnet_ref.forward(frames, weights)
    want = resnet_ref.forward64(frames, weights)
    assert got["output"].shape == got["correct"].shape == (1, 8, 16) and got["stems"].shape == (1, 8, 16, 64)
    err = np.abs(got["output"].astype(np.float64) - want["output"])
    print("max error %.3g, bound %.3g .. %.3g, max |output| %.3g" % (err.max(), want["bound"].min(), want["bound"].max(),
                                                                      np.abs(want["output"]).max()))
    assert (err <= want["bound"]).all(), (err.max(), want["bound"].min())
    assert err.max() > 0 and np.abs(want["output"]).max() > want["bound"].max()  # (two evaluations; and the bound says something)
    C.assert_same(got["correct"], want["correct"], "lidar_correct * scale_range")
