"""ResNet18Image and ResNet18ImageTrainable without a device: the layer table against the reference constructor's numbers, and
tests/resnet_image_ref.py held two ways: the identity (with img_conv zeroed it is ResNet18_NO_BN_l2's reference bit for bit, in
the outputs and in every shared layer's gradient) and float64 torch autograd of the same graph, by the method and the bound of
tests/test_resnet_train.py.  One frame of 8 x 8 throughout (level 4 is one pixel); every reference is worked out once."""
import importlib

import numpy as np
import pytest

import conv2_ref as R2
import conv_ref as R
import resnet_image_ref as RI
import resnet_ref
import resnetgrad_ref

F = np.float32
SHAPE = (1, 8, 8)
JOINT = (False, True)


@pytest.fixture(scope="module")
def net(pkg):
    return importlib.import_module(pkg.__name__ + ".net")


def batch():
    """(lidar, rgb, gt): a third of the pixels carry a LiDAR return of 1 .. 80 m, two thirds a ground truth near it; the image
    is what rgb_read emits, bytes / 255."""
    rng = np.random.default_rng(5)
    depth = rng.uniform(1, 80, SHAPE)
    lidar = np.where(rng.random(SHAPE) < 0.3, depth, 0).astype(F)
    gt = np.where(rng.random(SHAPE) < 0.65, depth + rng.normal(0, 0.5, SHAPE), 0).astype(F)
    rgb = (rng.integers(0, 256, SHAPE + (3,)).astype(F) / F(255.0)).astype(F)
    return lidar, rgb, gt


_cache = {}


def reference(net, zeroed):
    """(weights, {joint_train: grads}, forward, stats) of the image network on batch(), img_conv zeroed or not; once each."""
    if zeroed not in _cache:
        weights = net.glorot_weights_resnet18_image(7, 4, True, bias=0.1)
        if zeroed:
            weights["img_conv"] = tuple(np.zeros_like(a) for a in weights["img_conv"])
        lidar, rgb, gt = batch()
        _cache[zeroed] = (weights,) + RI.loss_gradients(lidar, rgb, gt, weights, joint_train=JOINT)
    return _cache[zeroed]


def test_the_layer_table_is_the_constructors(net):
    import torch

    for scale_num in (1, 2, 3, 4):
        for if_correct in (True, False):
            shapes = net.layer_shapes_resnet18_image(scale_num, if_correct)
            assert shapes == RI.layer_shapes(scale_num, if_correct), (scale_num, if_correct)
            plain = net.layer_shapes_resnet18(scale_num, if_correct)
            assert set(shapes) == set(plain) | {"img_conv"}
            differ = {n for n in plain if plain[n] != shapes[n]}
            assert differ == {"conv1a", "conv1a_extra", "upsample_1_post"}
            assert all(shapes[n][1] == plain[n][1] + 64 and shapes[n][::2] == plain[n][::2] for n in differ)
    assert net.layer_shapes_resnet18_image(4, True)["img_conv"] == (3, 3, 64)
    weights = net.glorot_weights_resnet18_image(1, 2, False)
    assert weights["img_conv"][0].shape == (3, 3, 3, 64) and weights["upsample_1_post"][0].shape == (3, 3, 160, 64)
    assert weights["upsample_3"][0].shape == (3, 3, 128, 256)  # a Conv2DTranspose: Keras' [3,3,Cout,Cin]
    model = net.ResNet18ImageTrainable(weights, if_correct=False, scale_num=2, joint_train=True)
    assert isinstance(model, torch.nn.Module) and isinstance(model, net.ResNet18Trainable)
    shapes = net.layer_shapes_resnet18_image(2, False)
    assert set(model.state_dict()) == {"%s.%s" % (n, v) for n in shapes for v in ("kernel", "bias")}
    assert tuple(model.img_conv.kernel.shape) == (3, 3, 3, 64) and tuple(model.conv1a.kernel.shape) == (3, 3, 96, 64)
    with pytest.raises(ValueError):
        net.ResNet18Image({k: v for k, v in weights.items() if k != "img_conv"}, if_correct=False, scale_num=2)
    with pytest.raises(ValueError):  # the plain network has no such layer
        net.ResNet18(weights, if_correct=False, scale_num=2)
    with pytest.raises(ValueError, match="image is data"):
        model(torch.zeros((1, 8, 8)), torch.zeros((1, 8, 8, 3), requires_grad=True))
    # the plain classes are what they were: no image width, the stems from channel 0
    assert net.ResNet18.IMAGE_WIDTH == 0 and net.ResNet18Image.IMAGE_WIDTH == 64
    assert net.ResNet18ImageTrainable._head is net.SparsityCNNTrainable._head


def test_with_a_zeroed_image_layer_it_is_the_plain_network(net):
    """img_conv's kernel and bias zero: its output is +0, the image's groups stand first in conv1a's and conv1a_extra's chains
    (and between upsample_1's and the stems' in upsample_1_post's) and add +-0, so the outputs and the gradient of every layer
    the two networks share are ResNet18_NO_BN_l2's, whose three kernels are the image network's with the image rows cut out."""
    weights, grads, fw, stats = reference(net, True)
    lidar, rgb, gt = batch()
    plain = RI.plain_weights(weights, 4)
    assert {n: (k.shape[0], k.shape[2], k.shape[3]) for n, (k, b) in plain.items() if n not in resnet_ref.TRANSPOSED and n != "lidar_conv_extra_3"} \
        == {n: s for n, s in net.layer_shapes_resnet18(4, True).items() if n not in resnet_ref.TRANSPOSED}
    want, want_fw, want_stats = resnetgrad_ref.loss_gradients(lidar, gt, plain, joint_train=JOINT)
    R.assert_same(fw["output"], want_fw["output"], "output")
    R.assert_same(fw["correct"], want_fw["correct"], "correct")
    R.assert_same(fw["stems"][..., 64:], want_fw["stems"], "the stems")
    assert (fw["stems"][..., :64] == 0).all() and np.abs(fw["output"]).max() > 0
    assert tuple(stats) == tuple(want_stats)
    for joint in JOINT:
        assert set(grads[joint]) == set(want[joint]) | {"img_conv"}
        for name, (dw, db) in want[joint].items():
            mine_dw, mine_db = grads[joint][name]
            if name in ("conv1a", "conv1a_extra"):
                mine_dw = mine_dw[:, :, 64:]
            elif name == "upsample_1_post":
                mine_dw = np.concatenate([mine_dw[:, :, :64], mine_dw[:, :, 128:]], axis=2)
            R.assert_same(mine_dw, dw, "d %s.kernel, joint_train %s" % (name, joint))
            R.assert_same(mine_db, db, "d %s.bias, joint_train %s" % (name, joint))
            assert (dw != 0).any(), name
        # an image layer that puts out zero under a leaky_relu still has a gradient: g = dy * alpha on y == 0
        assert (grads[joint]["img_conv"][0] != 0).any()
        # the image rows of the three kernels see x = 0: their gradient is zero
        assert (grads[joint]["conv1a"][0][:, :, :64] == 0).all() and (grads[joint]["upsample_1_post"][0][:, :, 64:128] == 0).all()


@pytest.mark.parametrize("joint_train", JOINT)
def test_resnet_image_ref_against_float64_autograd(net, joint_train):
    """tests/test_resnet_train.py's method and bound on the image network: the same graph in float64 torch operations under the
    tape, every leaky_relu on the branch the float32 forward took, each variable's gradient held to 1e-4 of its largest entry."""
    import torch
    import torch.nn.functional as TF

    import gmc_grad_ref

    weights, grads, fw, stats = reference(net, False)
    got = grads[joint_train]
    lidar, rgb, gt = batch()
    assert stats[2] > 20 and stats[3] > 5

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    var = {n: (t(k).requires_grad_(True), t(b).requires_grad_(True)) for n, (k, b) in weights.items()}
    alpha = float(F(0.2))
    calls = {name: 0 for name in fw["tape"]}

    def finish(y, name, act):
        call = fw["tape"][name][calls[name]]
        calls[name] += 1
        if not act:
            return y
        positive = torch.from_numpy(np.ascontiguousarray(call[1] > 0)).permute(0, 3, 1, 2)  # the float32 forward's branch
        return torch.where(positive, y, y * alpha)

    def conv(v, name, stride=1, residual=None, act=True):
        k, b = var[name]
        ksize = k.shape[0]
        (_, pt, pb), (_, pl, pr) = R2.same_rule(v.shape[2], ksize, stride), R2.same_rule(v.shape[3], ksize, stride)
        y = TF.conv2d(TF.pad(v, (pl, pr, pt, pb)), k.permute(3, 2, 0, 1).contiguous(), b, stride=stride)
        return finish(y if residual is None else y + residual, name, act)

    def up(v, name):
        k, b = var[name]  # Keras's [3,3,Cout,Cin]
        y = TF.conv_transpose2d(v, k.permute(3, 2, 0, 1).contiguous(), b, stride=2)[:, :, :2 * v.shape[2], :2 * v.shape[3]]
        return finish(y, name, True)

    x = t(lidar)
    mask = (x > float(F(0.1))).double()
    c = (x / 90.0)[:, None]
    for name in ("correct_1", "correct_2", "correct_3"):
        c = conv(c, name)
    correct = conv(c, "correct_4", act=False)[:, 0] * mask
    lidars = gmc_grad_ref.torch_statement(correct if joint_train else correct.detach(), mask, 7, 4)
    image = conv(t(rgb).permute(0, 3, 1, 2), "img_conv")
    stems = torch.cat([image] + [conv(l[:, None], name) for l, name in zip(lidars, ("lidar_conv", "lidar_conv_extra_1", "lidar_conv_extra_2",
                                                                                      "lidar_conv_extra_1"))], dim=1)
    below, totals = stems, []
    for level in (1, 2, 3, 4):
        name, stride = "conv%d" % level, 1 if level == 1 else 2
        a = conv(below, name + "a", stride)
        add = conv(below, name + "a_extra", stride, act=False)
        total = conv(a, name + "b", residual=add)
        below = conv(conv(total, name + "c"), name + "d", residual=total if level < 4 else None)
        totals.append(below)
    for level in (4, 3, 2):
        below = conv(torch.cat([up(below, "upsample_%d" % level), totals[level - 2]], dim=1), "upsample_%d_post" % level)
    z = conv(torch.cat([conv(below, "upsample_1"), stems], dim=1), "upsample_1_post")
    pred, corr = conv(z, "conv_output", act=False)[:, 0] * 90.0, correct * 90.0
    assert np.allclose(pred.detach().numpy(), fw["output"], rtol=1e-3, atol=1e-3)
    g64 = t(gt)
    with_gt = g64 > float(F(0.1))
    with_in = with_gt & (x > float(F(0.1)))
    total = ((pred - g64) ** 2 * with_gt).sum() / with_gt.sum() + \
        ((corr - g64) ** 2 * with_in + (corr - g64).abs() * with_in).sum() / with_in.sum()
    total.backward()
    assert set(got) == set(net.layer_shapes_resnet18_image(4, True))
    worst = max(np.abs(m - var[n][i].grad.numpy()).max() / np.abs(var[n][i].grad.numpy()).max() for n, pair in got.items() for i, m in enumerate(pair))
    print("largest error of a variable's gradient, in units of its largest entry: %.2e" % worst)
    for name, (dw, db) in got.items():
        assert dw.shape == weights[name][0].shape, name  # Keras' layout, the transposed layers' too
        for mine, want in ((dw, var[name][0].grad.numpy()), (db, var[name][1].grad.numpy())):
            scale = np.abs(want).max()
            assert scale > 0 and np.abs(mine - want).max() <= 1e-4 * scale, (name, np.abs(mine - want).max() / scale)
