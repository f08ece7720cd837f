"""ResNet18LightImageTrainable on the device: its forward against ResNet18LightImage bit for bit, the gradient of
train.py:240-251's loss with respect to every variable against tests/resnet_light_image_ref.py bit for bit (+0 == -0) with
joint_train both ways, the two-term rule on the tape itself, as tests/test_gpu_resnet_train.py checks it, and one optimizer step
without a host synchronisation.  One frame pair of 8 x 8 at scale_num 4 (level 4 is one pixel); the two settings of joint_train
share the numpy forward and everything behind the stems."""
import importlib

import numpy as np
import pytest

import conv_ref as C
import resnet_light_image_ref as RL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
SHAPE, SCALE_NUM = (2, 8, 8), 4


@pytest.fixture(scope="module")
def net(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".net")


def batch():
    """(lidar, rgb, gt): a third of the pixels carry a LiDAR return of 1 .. 80 m, two thirds a ground truth near it."""
    rng = np.random.default_rng(43)
    depth = rng.uniform(1, 80, SHAPE)
    lidar = np.where(rng.random(SHAPE) < 0.3, depth, 0).astype(F)
    gt = np.where(rng.random(SHAPE) < 0.65, depth + rng.normal(0, 0.5, SHAPE), 0).astype(F)
    rgb = (rng.integers(0, 256, SHAPE + (3,)).astype(F) / F(255.0)).astype(F)
    return lidar, rgb, gt


def _weights(net):
    return net.glorot_weights_resnet18_light_image(500 + SCALE_NUM, SCALE_NUM, True, bias=0.1)


_reference = []


def reference(net):
    """({joint_train: {layer: (dw, db)}}, forward, stats) by resnet_light_image_ref, once."""
    if not _reference:
        lidar, rgb, gt = batch()
        _reference.append(RL.loss_gradients(lidar, rgb, gt, _weights(net), joint_train=(False, True), scale_num=SCALE_NUM))
    return _reference[0]


def _tensors():
    import torch

    return [torch.from_numpy(a).to(DEV) for a in batch()]


def _step(pkg, model, lidar, rgb, gt):
    """train.py:232-253: the forward, the loss, backward().  Returns total."""
    output, correction = model(lidar, rgb)
    main, aux = pkg.autograd.train_loss(output, gt, lidar, correction)
    total = main + aux
    total.backward()
    return total


def test_forward_bits_are_the_inference_class(net):
    weights = _weights(net)
    lidar, rgb, _ = _tensors()
    want = [t.clone() for t in net.ResNet18LightImage(weights, scale_num=SCALE_NUM)(lidar, rgb)]
    model = net.ResNet18LightImageTrainable(weights, scale_num=SCALE_NUM).to(DEV)
    output, correct = model(lidar, rgb)
    assert output.requires_grad and correct.requires_grad
    C.assert_same(output.detach().cpu().numpy(), want[0].cpu().numpy(), "output * scale_range")
    C.assert_same(correct.detach().cpu().numpy(), want[1].cpu().numpy(), "lidar_correct * scale_range")
    C.assert_same(output.detach().cpu().numpy(), reference(net)[1]["output"], "output against resnet_light_image_ref")
    assert want[0].abs().max().item() > 0
    with pytest.raises(ValueError, match="image is data"):
        model(lidar, rgb.clone().requires_grad_())
    with pytest.raises(ValueError, match="input_rgb"):
        model(lidar, rgb[:1].contiguous())


@pytest.mark.parametrize("joint_train", (False, True))
def test_every_gradient_is_resnet_light_image_ref_bit_for_bit(pkg, net, joint_train):
    lidar, rgb, gt = _tensors()
    wants, fw, stats = reference(net)
    want = wants[joint_train]
    assert stats[2] > 50 and stats[3] > 10  # both losses have terms
    model = net.ResNet18LightImageTrainable(_weights(net), scale_num=SCALE_NUM, joint_train=joint_train).to(DEV)
    total = _step(pkg, model, lidar, rgb, gt)
    assert total.item() == F(F(stats[0]) + F(stats[1]))
    assert set(want) == set(net.layer_shapes_resnet18_light_image(SCALE_NUM, True))
    for name, p in model.named_parameters():
        layer, var = name.split(".")
        assert p.grad is not None, name + " has no gradient"
        C.assert_same(p.grad.cpu().numpy(), want[layer][var == "bias"], "d " + name)
        assert np.isfinite(want[layer][0]).all() and (want[layer][0] != 0).any(), name
    assert rgb.grad is None
    # a second backward() on the same batch doubles the gradients exactly (x + x is exact)
    _step(pkg, model, lidar, rgb, gt)
    for name, p in model.named_parameters():
        layer, var = name.split(".")
        C.assert_same(p.grad.cpu().numpy(), 2 * want[layer][var == "bias"], "twice: d " + name)


def test_every_gradient_sum_of_the_tape_has_two_terms(net):
    """No (node, output) of the autograd graph has more than two consumers: conv1_pre's output is read by the image concat and
    the pools through one view and by the last concat; the three pools are one node with three outputs, one consumer each."""
    lidar, rgb, _ = _tensors()
    model = net.ResNet18LightImageTrainable(_weights(net), scale_num=SCALE_NUM, joint_train=True).to(DEV)
    output, correct = model(lidar, rgb)
    uses, seen, todo = {}, set(), [output.grad_fn, correct.grad_fn]
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        for nxt, nr in node.next_functions:
            if nxt is not None:
                uses[(nxt, nr)] = uses.get((nxt, nr), 0) + 1
                todo.append(nxt)
    assert len(seen) > 100 and max(uses.values()) == 2
    three = [type(n).__name__ for (n, _), c in uses.items() if c > 2]
    assert not three, three
    pools = [n for n in seen if "MaxPoolPyramid" in type(n).__name__]
    assert len(pools) == 1 and all(uses[(pools[0], nr)] == 1 for nr in range(3))


def test_one_adam_step_without_a_host_synchronisation(pkg, net):
    """train.py:253-254 with torch.optim.Adam, as tests/test_gpu_resnet_train.py does it: every parameter moves, the loss on the
    same batch drops, and nothing between the forward and the optimizer's step blocks the host."""
    import torch

    lidar, rgb, gt = _tensors()
    model = net.ResNet18LightImageTrainable(_weights(net), scale_num=SCALE_NUM, joint_train=True).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-5, capturable=True)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    _step(pkg, model, lidar, rgb, gt)  # warm: the allocator's pools, the workspaces and Adam's state exist
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = _step(pkg, model, lidar, rgb, gt)
        opt.step()
        opt.zero_grad()
        with torch.no_grad():
            output, correction = model(lidar, rgb)
            main, aux = pkg.autograd.train_loss(output, gt, lidar, correction)
            after = main + aux
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[n]), n + " did not move"
    assert np.isfinite(after.item()) and after.item() < first.item(), (first.item(), after.item())
