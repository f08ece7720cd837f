"""ResNet18LightImage and ResNet18LightImageTrainable without a device: the layer table against the reference constructor's
numbers, and tests/resnet_light_image_ref.py held to float64 torch of the same graph: its forward within the bound of
tests/resnet_ref.py's forward64 (per-layer rounding bounds carried to the output through the float64 Jacobian), and its gradients
by the method and the bound of tests/test_resnet_image.py.  One frame of 8 x 8 throughout (level 4 is one pixel)."""
import importlib

import numpy as np
import pytest

import conv2_ref as R2
import conv_ref as R
import resnet_light_image_ref as RL
import resnet_ref

F = np.float32
SHAPE = (1, 8, 8)
JOINT = (False, True)
STEMS = ("lidar_conv", "lidar_conv_extra_1", "lidar_conv_extra_2", "lidar_conv_extra_1")


@pytest.fixture(scope="module")
def net(pkg):
    return importlib.import_module(pkg.__name__ + ".net")


def batch():
    """(lidar, rgb, gt) as tests/test_resnet_image.py draws them."""
    rng = np.random.default_rng(5)
    depth = rng.uniform(1, 80, SHAPE)
    lidar = np.where(rng.random(SHAPE) < 0.3, depth, 0).astype(F)
    gt = np.where(rng.random(SHAPE) < 0.65, depth + rng.normal(0, 0.5, SHAPE), 0).astype(F)
    rgb = (rng.integers(0, 256, SHAPE + (3,)).astype(F) / F(255.0)).astype(F)
    return lidar, rgb, gt


_cache = []


def reference(net):
    """(weights, {joint_train: grads}, forward, stats) on batch(), once."""
    if not _cache:
        weights = net.glorot_weights_resnet18_light_image(7, 4, True, bias=0.1)
        lidar, rgb, gt = batch()
        _cache.append((weights,) + RL.loss_gradients(lidar, rgb, gt, weights, joint_train=JOINT))
    return _cache[0]


def test_the_layer_table_is_the_constructors(net):
    import torch

    for scale_num in (1, 2, 3, 4):
        for if_correct in (True, False):
            shapes = net.layer_shapes_resnet18_light_image(scale_num, if_correct)
            assert shapes == RL.layer_shapes(scale_num, if_correct), (scale_num, if_correct)
            assert set(shapes) == set(net.layer_shapes_resnet18_image(scale_num, if_correct)) | {"conv1_pre"}
            assert all(cout in (1, 16, 64) for _, _, cout in shapes.values())
    shapes = net.layer_shapes_resnet18_light_image(4, True)
    assert shapes["conv1_pre"] == (3, 64, 64) and shapes["upsample_4"] == (3, 128, 64) and shapes["upsample_3_post"] == (3, 192, 64)
    weights = net.glorot_weights_resnet18_light_image(1, 2, False)
    assert weights["conv1_pre"][0].shape == (3, 3, 32, 64) and weights["conv4a_extra"][0].shape == (1, 1, 128, 64)
    assert weights["upsample_4"][0].shape == (3, 3, 64, 128)  # a Conv2DTranspose: Keras' [3,3,Cout,Cin]
    model = net.ResNet18LightImageTrainable(weights, if_correct=False, scale_num=2, joint_train=True)
    assert isinstance(model, torch.nn.Module) and isinstance(model, net.ResNet18ImageTrainable)
    shapes = net.layer_shapes_resnet18_light_image(2, False)
    assert set(model.state_dict()) == {"%s.%s" % (n, v) for n in shapes for v in ("kernel", "bias")}
    assert tuple(model.conv1_pre.kernel.shape) == (3, 3, 32, 64) and tuple(model.upsample_4.kernel.shape) == (3, 3, 64, 128)
    with pytest.raises(ValueError):
        net.ResNet18LightImage({k: v for k, v in weights.items() if k != "conv1_pre"}, if_correct=False, scale_num=2)
    with pytest.raises(ValueError):  # the wide network's weights do not fit
        net.ResNet18LightImage(net.glorot_weights_resnet18_image(1, 2, False), if_correct=False, scale_num=2)
    with pytest.raises(ValueError, match="image is data"):
        model(torch.zeros((1, 8, 8)), torch.zeros((1, 8, 8, 3), requires_grad=True))
    # the classes that were here are what they were
    assert net.ResNet18Image.NAME == "ResNet18_NO_BN_l2_image" and net.ResNet18LightImage.NAME == "ResNet18_NO_BN_l2_light_image"
    assert "conv1_pre" not in net.ResNet18Image.KNOWN and "conv1_pre" in net.ResNet18LightImage.KNOWN


def test_the_reference_wires_what_call_wires(net):
    """The tensors call() builds, by their widths and their contents: the pooled channels are pool_ref's of conv1_pre's output."""
    import pool_ref

    weights, grads, fw, stats = reference(net)
    assert fw["total"].shape == SHAPE + (64,) and fw["total1"].shape == SHAPE + (128,)
    assert (fw["total1"][..., 64:] == fw["total"]).all() and (fw["total"] < 0).any()  # conv1_pre is linear: no leaky_relu cut
    for level, k in ((2, 2), (3, 4), (4, 8)):
        assert fw["pooled"][level].shape == (1, 8 // k, 8 // k, 128)
        assert (fw["pooled"][level][..., 64:] == pool_ref.max_pool(fw["total"], k)).all()
    tape = fw["tape"]
    assert tape["upsample_4"][0][0].shape[-1] == 128 and tape["upsample_4_post"][0][0].shape[-1] == 192
    assert tape["conv4d"][0][4] is False and tape["conv3d"][0][4] is True  # level 4 has no second residual
    assert (tape["upsample_1_post"][0][0][..., 64:] == fw["total"]).all()  # the last concat takes lidar_conv_total, not the stems
    assert set(tape) == set(net.layer_shapes_resnet18_light_image(4, True)) and len(tape["lidar_conv_extra_1"]) == 2


def _graph64(weights, fw, stems, image, probes=None):
    """The graph from the stems' concat and img_conv's output on in float64 torch, every leaky_relu on the side the float32
    forward took.  probes: a list that receives (a zero added to each layer's y, the layer's rounding bound d) per layer, as
    tests/resnet_ref.py's forward64 does."""
    import torch
    import torch.nn.functional as TF

    alpha = float(F(0.2))
    calls = {name: 0 for name in fw["tape"]}

    def raw(v, k, stride, transposed):
        if transposed:  # Keras's [3,3,Cout,Cin]
            return TF.conv_transpose2d(v, k.permute(3, 2, 0, 1).contiguous(), stride=2)[:, :, :2 * v.shape[2], :2 * v.shape[3]]
        ksize = k.shape[0]
        (_, pt, pb), (_, pl, pr) = R2.same_rule(v.shape[2], ksize, stride), R2.same_rule(v.shape[3], ksize, stride)
        return TF.conv2d(TF.pad(v, (pl, pr, pt, pb)), k.permute(3, 2, 0, 1).contiguous(), stride=stride)

    def layer(v, name, stride=1, residual=None, act=True):
        k, b = weights[name]
        transposed = name in resnet_ref.TRANSPOSED
        bias = b.view(1, -1, 1, 1)
        y = raw(v, k, stride, transposed) + bias
        if residual is not None:
            y = y + residual
        if probes is not None:
            with torch.no_grad():
                size = raw(v.abs(), k.abs(), stride, transposed) + bias.abs() + (0 if residual is None else residual.abs())
            probe = torch.zeros_like(y, requires_grad=True)
            links = (4 if transposed else k.shape[0] ** 2) * v.shape[1]
            probes.append((probe, R.gamma(links + 3) * size))
            y = y + probe
        call = fw["tape"][name][calls[name]]
        calls[name] += 1
        if not act:
            return y
        positive = torch.from_numpy(np.ascontiguousarray(call[1] > 0)).permute(0, 3, 1, 2)
        return torch.where(positive, y, y * alpha)

    total = layer(stems, "conv1_pre", act=False)
    below, totals = torch.cat([image, total], dim=1), []
    for level in (1, 2, 3, 4):
        name, stride = "conv%d" % level, 1 if level == 1 else 2
        a = layer(below, name + "a", stride)
        add = layer(below, name + "a_extra", stride, act=False)
        mid = layer(a, name + "b", residual=add)
        below = layer(layer(mid, name + "c"), name + "d", residual=mid if level < 4 else None)
        if level > 1:
            below = torch.cat([below, TF.max_pool2d(total, 1 << (level - 1))], dim=1)
        totals.append(below)
    for level in (4, 3, 2):
        below = layer(torch.cat([layer(below, "upsample_%d" % level), totals[level - 2]], dim=1), "upsample_%d_post" % level)
    z = layer(torch.cat([layer(below, "upsample_1"), total], dim=1), "upsample_1_post")
    return layer(z, "conv_output", act=False)[:, 0]


def test_the_reference_forward_lies_within_the_derived_bound_of_float64(net):
    """resnet_ref.forward64's bound on this graph: the float32 head's stems and image layer as inputs, every later layer's
    rounding bound gamma(K + 3) (conv(|v|, |w|) + |bias| + |residual|) carried to the output by the float64 Jacobian, doubled
    for the second-order terms.  The pools round nothing."""
    import torch

    weights, grads, fw, stats = reference(net)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    var = {n: (t64(k), t64(b)) for n, (k, b) in weights.items()}
    image = fw["tape"]["img_conv"][0][1]
    probes = []
    out = _graph64(var, fw, t64(fw["stems"]).permute(0, 3, 1, 2), t64(image).permute(0, 3, 1, 2), probes)
    flat, first_order = out.reshape(-1), []
    for p in range(flat.numel()):
        g = torch.autograd.grad(flat[p], [probe for probe, _ in probes], retain_graph=True)
        first_order.append(sum(float((gi.abs() * d).sum()) for gi, (_, d) in zip(g, probes)))
    out = out.detach().numpy()
    r = np.float64(F(90.0))
    bound = 2 * np.array(first_order).reshape(out.shape) * r + R.gamma(1) * np.abs(out) * r
    err = np.abs(fw["output"].astype(np.float64) - out * r)
    print("largest error %.3e, its bound %.3e, largest output %.3e" % (err.max(), bound.flat[err.argmax()], np.abs(out * r).max()))
    assert len(probes) == 30 and (err <= bound).all() and np.abs(out).max() > 0
    assert err.max() > 0 and np.abs(out * r).max() > bound.max()  # (two evaluations; and the bound says something, as in test_resnet.py)


@pytest.mark.parametrize("joint_train", JOINT)
def test_the_reference_gradients_against_float64_autograd(net, joint_train):
    """tests/test_resnet_image.py's method and bound: the whole graph in float64 under torch's tape, each variable's gradient held
    to 1e-4 of its largest entry.  torch's max_pool2d routes a gradient to the one maximum of a window; the values here have no
    ties."""
    import torch

    import gmc_grad_ref

    weights, grads, fw, stats = reference(net)
    got = grads[joint_train]
    lidar, rgb, gt = batch()
    assert stats[2] > 20 and stats[3] > 5
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    var = {n: (t(k).requires_grad_(True), t(b).requires_grad_(True)) for n, (k, b) in weights.items()}
    alpha = float(F(0.2))
    calls = {name: 0 for name in ("correct_1", "correct_2", "correct_3", "correct_4", "img_conv") + STEMS}

    def conv(v, name, act=True):  # the head's layers and img_conv: stride 1, as _graph64's
        k, b = var[name]
        r = k.shape[0] // 2
        y = torch.nn.functional.conv2d(v, k.permute(3, 2, 0, 1).contiguous(), b, padding=r)
        call = fw["tape"][name][calls[name]]
        calls[name] += 1
        if not act:
            return y
        return torch.where(torch.from_numpy(np.ascontiguousarray(call[1] > 0)).permute(0, 3, 1, 2), y, y * alpha)

    x = t(lidar)
    mask = (x > float(F(0.1))).double()
    c = (x / 90.0)[:, None]
    for name in ("correct_1", "correct_2", "correct_3"):
        c = conv(c, name)
    correct = conv(c, "correct_4", act=False)[:, 0] * mask
    lidars = gmc_grad_ref.torch_statement(correct if joint_train else correct.detach(), mask, 7, 4)
    image = conv(t(rgb).permute(0, 3, 1, 2), "img_conv")
    stems = torch.cat([conv(l[:, None], name) for l, name in zip(lidars, STEMS)], dim=1)
    trunk = {n: v for n, v in var.items() if n not in calls}
    trunk_fw = dict(fw, tape={n: c for n, c in fw["tape"].items() if n not in calls})
    pred, corr = _graph64(trunk, trunk_fw, stems, image) * 90.0, correct * 90.0
    assert np.allclose(pred.detach().numpy(), fw["output"], rtol=1e-3, atol=1e-3)
    g64 = t(gt)
    with_gt = g64 > float(F(0.1))
    with_in = with_gt & (x > float(F(0.1)))
    total = ((pred - g64) ** 2 * with_gt).sum() / with_gt.sum() + \
        ((corr - g64) ** 2 * with_in + (corr - g64).abs() * with_in).sum() / with_in.sum()
    total.backward()
    assert set(got) == set(net.layer_shapes_resnet18_light_image(4, True))
    worst = max(np.abs(m - var[n][i].grad.numpy()).max() / np.abs(var[n][i].grad.numpy()).max() for n, pair in got.items() for i, m in enumerate(pair))
    print("largest error of a variable's gradient, in units of its largest entry: %.2e" % worst)
    for name, (dw, db) in got.items():
        assert dw.shape == weights[name][0].shape, name  # Keras' layout, the transposed layers' too
        for mine, want in ((dw, var[name][0].grad.numpy()), (db, var[name][1].grad.numpy())):
            scale = np.abs(want).max()
            assert scale > 0 and np.abs(mine - want).max() <= 1e-4 * scale, (name, np.abs(mine - want).max() / scale)
