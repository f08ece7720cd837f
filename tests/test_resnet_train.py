"""ResNet18Trainable without a device: its parameters against layer_shapes_resnet18, tests/resnetgrad_ref.py against float64
autograd of the same graph, and the two-term rule in the reference's bookkeeping (the tape itself is walked in
tests/test_gpu_resnet_train.py: the module's operators run on the device only)."""
import importlib

import numpy as np
import pytest

import conv2_ref as R2
import conv_ref as R
import resnetgrad_ref

F = np.float32


@pytest.fixture(scope="module")
def net(pkg):
    return importlib.import_module(pkg.__name__ + ".net")


def test_parameters_are_the_references_variables(net):
    import torch

    for scale_num, if_correct in ((4, True), (1, False)):
        shapes = net.layer_shapes_resnet18(scale_num, if_correct)
        weights = net.glorot_weights_resnet18(1, scale_num, if_correct)
        model = net.ResNet18Trainable(weights, if_correct=if_correct, scale_num=scale_num, joint_train=True)
        assert isinstance(model, torch.nn.Module) and model.joint_train
        assert set(model.state_dict()) == {"%s.%s" % (n, v) for n in shapes for v in ("kernel", "bias")}
        for name, (k, cin, cout) in shapes.items():
            keras = (k, k, cout, cin) if name in net.RESNET_TRANSPOSED else (k, k, cin, cout)  # Keras' layouts, not the packed one
            assert tuple(getattr(model, name).kernel.shape) == keras and tuple(getattr(model, name).bias.shape) == (cout,), name
            assert np.array_equal(getattr(model, name).kernel.detach().numpy(), weights[name][0]), name
        assert not hasattr(model, "lidar_conv_extra_3")
    assert tuple(model.upsample_4.kernel.shape) == (3, 3, 256, 512)
    weights = net.glorot_weights_resnet18(1)
    with pytest.raises(ValueError):
        net.ResNet18Trainable({k: v for k, v in weights.items() if k != "conv3b"})
    with pytest.raises(ValueError):
        net.ResNet18Trainable(weights, scale_num=5)
    with pytest.raises(ValueError, match="multiples of 8"):
        net.ResNet18Trainable(weights)(torch.zeros((1, 12, 16)))
    # the factored head is one statement for both trainable networks
    assert net.ResNet18Trainable._head is net.SparsityCNNTrainable._head
    assert "weight-decay" in net.ResNet18Trainable.__doc__


def test_the_two_term_rule_in_the_references_bookkeeping():
    """Four tensors have three consumers; each gradient is (d conv_a + d conv_a_extra) + d concat, two two-term sums."""
    want = {"stems": (("conv1a", "conv1a_extra"), "concat_1")}
    for k in (1, 2, 3):
        want["tensor_%d_total" % k] = (("conv%da" % (k + 1), "conv%da_extra" % (k + 1)), "concat_%d" % (k + 1))
    assert resnetgrad_ref.CONSUMERS == want
    for nest in resnetgrad_ref.CONSUMERS.values():
        assert len(nest) == 2 and len(nest[0]) == 2 and isinstance(nest[1], str)
    # a float32 sum of three terms does depend on its grouping: the rule is not idle
    u = F(2.0 ** -24)
    assert (F(1) + u) + u != F(1) + (u + u)


@pytest.mark.parametrize("joint_train", (False, True))
def test_resnetgrad_ref_against_float64_autograd(net, joint_train):
    """The same graph in float64 torch operations under the tape (F.conv2d on the 'same' rule's padding, conv_transpose2d cropped,
    gmc_grad_ref.torch_statement for the fill, train.py's loss expression), on a frame of 8 x 8 (level 4 is one pixel).  Every
    leaky_relu of the float64 graph takes the branch the float32 forward took (the tape's outputs decide it), so the two sides
    differentiate the same piecewise-linear function and a float32 value that a rounding moved across zero cannot make the
    comparison a comparison of two different functions.  The net is a composition of some thirty chains, so its gradient's
    error is not one gamma: as in test_conv2d_backward's netgrad test, each variable's gradient is held to 1e-4 of its largest
    entry, four digits where float32 carries seven, which a wrong term (a consumer left out of a three-consumer sum, a flip
    where an exchange belongs, a transposed kernel's gradient in the packed layout) misses by orders of magnitude."""
    import torch
    import torch.nn.functional as TF

    import gmc_grad_ref

    B, H, W = 2, 8, 8
    rng = np.random.default_rng(3)
    depth = rng.uniform(1, 80, (B, H, W))
    lidar = np.where(rng.random((B, H, W)) < 0.3, depth, 0).astype(F)
    gt = np.where(rng.random((B, H, W)) < 0.65, depth + rng.normal(0, 0.5, (B, H, W)), 0).astype(F)
    weights = net.glorot_weights_resnet18(7, 4, True, bias=0.1)
    got, fw, stats = resnetgrad_ref.loss_gradients(lidar, gt, weights, joint_train=joint_train)
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
    for a, b in zip(lidars, fw["lidars"]):
        assert np.array_equal(a.detach().numpy() > 0.001, b > F(0.001)) and np.allclose(a.detach().numpy(), b, rtol=1e-4, atol=1e-6)
    stems = torch.cat([conv(l[:, None], name) for l, name in zip(lidars, ("lidar_conv", "lidar_conv_extra_1", "lidar_conv_extra_2",
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
    assert set(got) == set(net.layer_shapes_resnet18(4, True))
    worst = max(np.abs(m - var[n][i].grad.numpy()).max() / np.abs(var[n][i].grad.numpy()).max() for n, pair in got.items() for i, m in enumerate(pair))
    print("largest error of a variable's gradient, in units of its largest entry: %.2e" % worst)
    for name, (dw, db) in got.items():
        assert dw.shape == weights[name][0].shape, name  # Keras' layout, the transposed layers' too
        for mine, want in ((dw, var[name][0].grad.numpy()), (db, var[name][1].grad.numpy())):
            scale = np.abs(want).max()
            assert scale > 0 and np.abs(mine - want).max() <= 1e-4 * scale, (name, np.abs(mine - want).max() / scale)
